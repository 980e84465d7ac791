# Diagnostic: the bench line (end-to-end and other-workload figures included) under each LACX_STREAM_PRIO setting.
#   scripts/prio_ab.sh [out_dir]      (default: a fresh temporary directory, printed at the end)
OUT=${1:-$(mktemp -d)}
mkdir -p "$OUT"
for P in "0,1,-1" "-1,1,0" "-1,0,1" "-1,1,-1"; do
  LACX_STREAM_PRIO=$P python bench.py --full --no-cpu-baseline --no-decode-check > "$OUT/b_$P.json" 2> "$OUT/b_$P.err"
done
echo "$OUT"
