// CPU check of rtw_render_adaptive's checkpoint schedule and argument validation (raytracing_weekend_amd/csrc/rtw_plan.h
// adaptive_checkpoints): run by tests/test_adaptive_cpu.py, which compares what this prints with tests/adaptive_ref.py.
// Each line: "ok <min> <step> <cap> : n_0 n_1 ..." or "bad <min> <step> <cap> <threshold> <dilate>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_plan.h"

int main(int argc, char** argv) {
    // arguments: groups of five (min_spp step_spp cap threshold dilate)
    for (int i = 1; i + 4 < argc; i += 5) {
        const int mn = atoi(argv[i]), st = atoi(argv[i + 1]), cap = atoi(argv[i + 2]), dil = atoi(argv[i + 4]);
        const float thr = (float)atof(argv[i + 3]);
        std::vector<int> cps;
        const char* why = rtwk::adaptive_checkpoints(mn, st, cap, thr, dil, cps);
        if (why) {
            printf("bad %d %d %d %s %d\n", mn, st, cap, argv[i + 3], dil);
            continue;
        }
        printf("ok %d %d %d :", mn, st, cap);
        for (int n : cps) printf(" %d", n);
        printf("\n");
    }
    return 0;
}
