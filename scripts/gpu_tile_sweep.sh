cd $GRAFT_REPO_ROOT
export OUT_DIR=${OUT_DIR:-prof_out}
mkdir -p $OUT_DIR
for t in 4096 8192 12288 16384 32768; do
  python bench.py --full --no-cpu --no-c4 --no-c5 --tile-docs $t 2>/dev/null > $OUT_DIR/ts_$t.json
  python - $t <<'PY'
import sys, json, os
O = os.environ['OUT_DIR']
d = json.loads(open(f"{O}/ts_{sys.argv[1]}.json").read())
print("tile", sys.argv[1], "flickr_ms", d["ms_per_step"], "qps", round(d["value"]), "kernel_ms", d["roofline"]["kernel_ms"])
PY
done
