#!/usr/bin/env bash
# tools/synth_traffic.sh -- HBM traffic counters of synth_block_v1 (one rocprofv3 --pmc run per pass,
# kernel trace only, never combined with other tracing) over tools/synth_ab.py's fused path, in the
# layout tools/pmc_traffic.py reads.  Any failure ends the script (no retries).
# Usage (repo root): [PMC_DIR=dir] bash tools/synth_traffic.sh [instances] [steps]
#   then: [PMC_DIR=dir] python tools/pmc_traffic.py synth <instances> 256 synth_block --out profiles/traffic_synth.json
# PMC_DIR: where the passes are written and read (default pmc_out/pmc_synth)
set -u
n=${1:-16384}; steps=${2:-10}
out=${PMC_DIR:-pmc_out/pmc_synth}
mkdir -p "$out"
export TMPDIR=/tmp PYTHONUNBUFFERED=1
sha256sum ol_dsp_amd/libolfx.so | cut -d' ' -f1 > "$out/libolfx.sha256"
passes=(
  "FETCH_SIZE"
  "WRITE_SIZE"
  "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum"
  "TCC_EA0_RDREQ_64B_sum TCC_EA0_RDREQ_128B_sum"
  "TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum"
)
k=0
for p in "${passes[@]}"; do
  k=$((k+1))
  echo "== pass $k: $p"
  timeout -k 10 300 rocprofv3 --kernel-trace --kernel-include-regex "synth_block" --pmc $p -d "$out/p$k" -o run --output-format csv -- \
      python3 tools/synth_ab.py --only fused --instances "$n" --steps "$steps" --warmup 2 > "$out/p$k.log" 2>&1
  rc=$?
  echo "   rc=$rc"
  if [ $rc -ne 0 ]; then tail -5 "$out/p$k.log"; exit $rc; fi
done
echo "== done"
