// PfmWriter.h — Portable Float Map output shared by the Director's beauty file and its guide files (-aov).
#pragma once
#include <fstream>
#include <string>
#include <vector>

namespace rtwhost {

// "PF" (channels = 3) or "Pf" (channels = 1), little-endian (scale -1.0). PFM rows run bottom-up, like the frame buffer: row 0 of
// `data` (the image's bottom row) is written first. data: width*height pixels of `stride` floats, of which the first `channels`
// are written.
inline bool writePfm(const std::string& path, const float* data, int width, int height, int stride, int channels) {
    if (channels != 1 && channels != 3) return false;
    std::ofstream f(path, std::ios::binary);
    if (!f) return false;
    f << (channels == 3 ? "PF\n" : "Pf\n") << width << " " << height << "\n-1.0\n";
    std::vector<float> row(static_cast<size_t>(width) * channels);
    for (int j = 0; j < height; j++) {
        for (int i = 0; i < width; i++) {
            const float* px = &data[(static_cast<size_t>(width) * j + i) * stride];
            for (int k = 0; k < channels; k++) row[static_cast<size_t>(channels) * i + k] = px[k];
        }
        f.write(reinterpret_cast<const char*>(row.data()), static_cast<std::streamsize>(row.size() * sizeof(float)));
    }
    return static_cast<bool>(f);
}

}  // namespace rtwhost
