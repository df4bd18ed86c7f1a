#!/bin/bash
# usage: [NEE1=0|1] [SHAPE=0|1] scripts/isa_phases.sh [extra flags] : static instruction counts of the shipped k_path<PHILOX,0,0,0,NEE1,SHAPE>
# per phase (between the phase-fence comments; NEE1 = 1 with SHAPE = 1, the defaults, is the one-light instantiation with the Cornell box's
# fixed-shape walks that the headline scene runs; SHAPE = 0 with NEE1 = 1 the one-light instantiation other one-light scenes run). Compiles
# rtw_inst_path.hip with __graft_entry__.unit_flags (HIP_FLAGS + that unit's UNIT_FLAGS) and prints, per phase, the instruction classes and the reciprocal / root sequences: div = the compiler's correctly rounded
# divisions (v_div_fixup_f32, fallbacks of the short forms included), sqrt = its roots (v_sqrt_f32), rcp_short / rsq_short = the
# short forms of rtw_math.h (a v_rcp_f32 without a v_div_fixup_f32; v_rsq_f32). Exits 1 when the kernel is not found.
R=$(cd "$(dirname "$0")/.." && pwd)
NEE1=${NEE1:-1}
K=_ZN4rtwk6k_pathILi0ELi0ELi0ELi0ELi${NEE1}ELi${SHAPE:-$NEE1}EEEvNS_5KArgsE
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
FLAGS=$(cd "$R" && python3 -c "
import __graft_entry__ as g
print(' '.join(g.unit_flags('rtw_inst_path.hip')))") || exit 1
${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS "$@" -S --cuda-device-only -o "$T/rtw.s" "$R/raytracing_weekend_amd/csrc/rtw_inst_path.hip" || exit 1
awk '/^'$K':/{f=1} f{print} /s_endpgm/{if(f){exit}}' "$T/rtw.s" > "$T/kpath.s"
if [ ! -s "$T/kpath.s" ]; then echo "isa_phases: no $K in the assembly" >&2; exit 1; fi
awk '/\.amdhsa_kernel '$K'/{f=1} f&&/amdhsa_next_free_vgpr|amdhsa_private_segment_fixed_size/{print} /\.end_amdhsa_kernel/{f=0}' "$T/rtw.s"
awk '/^'$K':/{f=1} f&&/^; codeLenInByte/{print; exit}' "$T/rtw.s"
python3 - "$T/kpath.s" <<'PY'
import re,collections,sys
cur="pre"; cnt=collections.OrderedDict()
for l in open(sys.argv[1]):
    l=l.strip()
    m=re.match(r"; MARK (\w+)",l)
    if m: cur=m.group(1); continue
    if not l or l.startswith(';') or l.startswith('.') or l.endswith(':'): continue
    op=l.split()[0]
    c=cnt.setdefault(cur,collections.Counter())
    if op.startswith('v_'): c['valu']+=1
    elif op.startswith('s_load') or op.startswith('s_buffer'): c['smem']+=1
    elif op.startswith('s_cbranch') or op.startswith('s_branch'): c['branch']+=1
    elif op.startswith('s_waitcnt'): c['wait']+=1
    elif op.startswith('s_'): c['salu']+=1
    elif op.startswith('ds_'): c['lds']+=1
    elif op.startswith(('global_','scratch_','buffer_','flat_')): c['vmem']+=1
    if op.startswith('v_mov'): c['v_mov']+=1
    if op.startswith(('v_readlane','v_writelane')): c['lane']+=1
    if op.startswith('v_readlane'): c['readlane']+=1
    if op.startswith('v_readfirstlane'): c['readfirstlane']+=1
    if op.startswith('scratch_'): c['scratch']+=1
    if op.startswith('v_mad_u64_u32'): c['mad_u64']+=1
    if op.startswith('v_cndmask'): c['cndmask']+=1
    if op.startswith('v_cmp'): c['cmp']+=1
    if op.startswith('v_div_fixup_f32'): c['div']+=1
    if op.startswith('v_sqrt_f32'): c['sqrt']+=1
    if op.startswith('v_rcp_f32'): c['rcp']+=1
    if op.startswith('v_rsq_f32'): c['rsq_short']+=1
tot=collections.Counter()
for k,v in cnt.items():
    v['rcp_short']=v.pop('rcp',0)-v.get('div',0)
    tot.update(v)
    print(k, dict(v))
print('total', dict(tot))
PY
