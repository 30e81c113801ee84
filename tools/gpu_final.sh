# Round check: every -m gpu test, smoke, the full bench line (each under its own limit)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${1:?usage: gpu_final.sh OUTPUT_DIR} && mkdir -p "$out" || exit 9
timeout -k 10 900 python -u -m pytest -x -v --timeout 300 --timeout-method thread tests -m gpu > "$out/fin_tests.log" 2>&1 || exit 1
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > "$out/fin_smoke.log" 2>&1 || exit 2
timeout -k 10 600 python -u bench.py --full > "$out/fin_bench.json" 2> "$out/fin_bench.err" || exit 3
