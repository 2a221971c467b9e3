# Unprofiled same-box A/B of prebuilt library variants (tools/ab_build.sh) on the headline bench: variants interleaved, ROUNDS rounds,
# one bench.py process each (200-step regions, median of 5).  usage: ROUNDS=2 tools/ab_bench.sh default tagA tagB ...   [BENCH_ARGS=...]
# Every run has a time limit of its own (RUN_LIMIT seconds, default: sized from the run -- start-up and warm-up, then STEPS x REPEATS
# steps at a generous 5 ms each, twice for the single-stream pass) and the script stops at the first run that fails or times out:
# nothing more is started on a GPU that a run has left in doubt.  The default library is put back on every way out.
# (The variants share the Python binding of this tree: a library of another ABI is measured from a checkout of its own commit.)
R=${ROUNDS:-2}
STEPS=200; REPEATS=5
LIMIT=${RUN_LIMIT:-$((120 + 2 * STEPS * REPEATS * 5 / 1000))}
mkdir -p cips_3dplusplus_amd/_ab
if [ ! -f cips_3dplusplus_amd/_ab/lib_default.so ]; then
  python3 -m cips_3dplusplus_amd.build > /dev/null 2>&1 || { echo "build of the default library failed"; exit 1; }
  cp cips_3dplusplus_amd/libcips3d_hip.so cips_3dplusplus_amd/_ab/lib_default.so
  cp cips_3dplusplus_amd/libcips3d_hip.so.srchash cips_3dplusplus_amd/_ab/hash_default; : > cips_3dplusplus_amd/_ab/flags_default
fi
restore() { cp cips_3dplusplus_amd/_ab/lib_default.so cips_3dplusplus_amd/libcips3d_hip.so; cp cips_3dplusplus_amd/_ab/hash_default cips_3dplusplus_amd/libcips3d_hip.so.srchash; }
trap restore EXIT
for i in $(seq $R); do
  for v in "$@"; do
    cp cips_3dplusplus_amd/_ab/lib_$v.so cips_3dplusplus_amd/libcips3d_hip.so || exit 1
    cp cips_3dplusplus_amd/_ab/hash_$v cips_3dplusplus_amd/libcips3d_hip.so.srchash || exit 1
    OUT=$(CIPS3D_HIPCC_FLAGS="$(cat cips_3dplusplus_amd/_ab/flags_$v)" timeout -k 10 $LIMIT python3 bench.py --full --no-also --no-cpu-baseline --steps $STEPS --repeats $REPEATS --detail "" ${BENCH_ARGS} 2>/dev/null)
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v: bench.py ended with status $rc in round $i (limit ${LIMIT} s): stopping"; exit $rc; fi
    echo -n "$v: "
    echo "$OUT" | tail -1 | \
      python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['ms_per_step'], d['ms_per_step_repeats'], 'single_stream', (d.get('single_stream') or {}).get('ms_per_step'), 'render', d['roofline']['avg_launch_ms'])" || exit 1
  done
done
