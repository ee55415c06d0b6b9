# per-shape GEMM times (eager HIP events, XGGM_DUMP_GEMMS) with the grouped tile pinned: which launches want which tile.
# XGGM_TILE_TABLE=0: without it the signatures of the measured table keep their table tile (a launch's own tile wins over
# the process-wide pin) and only the other launches run under the tile named here.
OUT=${1:?usage: tools/exp_group_tile.sh OUTPUT_DIR}
mkdir -p "$OUT"
for t in 0 1 2 4; do
  XGGM_DUMP_GEMMS=1 XGGM_TILE_TABLE=0 XGGM_GROUP_TILE=$t python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-loader --no-ref-batch > /dev/null 2> "$OUT/dump_tile$t.txt"
done
grep -c gemm "$OUT/dump_tile0.txt"
