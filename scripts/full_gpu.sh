# the round-end checks in one call: every -m gpu test, smoke(), the default bench line with
# its extras (--full: copy floor, CPU baseline, parity).  Logs under $NUT_OUT_DIR (default bench_out/).
cd "${NUT_REPO_ROOT:-$(dirname "$0")/..}" && export NUT_PREBUILT=1
out=${NUT_OUT_DIR:-bench_out}
mkdir -p "$out"
timeout -k 10 1000 python -u -m pytest tests -m gpu -q --timeout 400 --timeout-method thread > "$out/t_all.log" 2>&1; rc=$?
tail -4 "$out/t_all.log"
[ $rc = 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$out/smoke.log" 2>&1 || { tail -5 "$out/smoke.log"; exit 1; }
tail -1 "$out/smoke.log"
timeout -k 10 300 python bench.py --full > "$out/bench_default.log" 2>&1 || { tail -5 "$out/bench_default.log"; exit 1; }
grep '^{' "$out/bench_default.log" | tail -1 | cut -c1-400
