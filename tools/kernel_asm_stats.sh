#!/bin/bash
# Dev tool: compile one translation unit of deepmod_amd/csrc/ to gfx950 assembly (with extra -D flags) and print the instruction mix, register use
# and spills of one of its kernels.   bash tools/kernel_asm_stats.sh unit kernel-name-substring [-DFLAG ...]
#   e.g. kern_f16q0.hip bilstm_f16q     feed.hip signal_norm_batch     offline.hip grad_kernel
[ $# -ge 2 ] || { echo "usage: $0 unit kernel-name-substring [-DFLAG ...]"; exit 2; }
U=$1; K=$2; shift 2
R=$(cd "$(dirname "$0")/.." && pwd)
S=$(mktemp /tmp/dmasm.XXXXXX.s)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form --cuda-device-only -S -o $S "$@" $R/deepmod_amd/csrc/$U 2>/dev/null || { echo "compile failed"; exit 1; }
awk -v k="$K" '/^_Z[A-Za-z0-9_]*:/ {on = index($0, k) > 0} on {print} on && /s_endpgm/ {exit}' $S > $S.k
echo "instructions: $(grep -E '^\s+[a-z]' $S.k | grep -v '^\s*;' | grep -vE '^\s+\.' | wc -l)"
grep -E "^\s+[vsdg][a-z_0-9]+" -o $S.k | sed 's/^\s*//' | sort | uniq -c | sort -rn | head -${TOP:-16}
awk -v k="$K" '$0 ~ "\\.name:.*" k {on=1} on && /vgpr_count|spill_count|sgpr_count/ {print} on && /wavefront_size/ {exit}' $S
[ -n "$KEEP" ] && cp $S.k $KEEP
rm -f $S $S.k
