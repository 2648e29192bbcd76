#!/bin/bash
# Accuracy session: the conv accuracy probe, the FRCNN stage- and layer-error tables, then (TESTS=1) the GPU
# parity tests and (BENCH=1) the bench at the driver's arguments.  Stops on a fault or time limit.
cd "$GRAFT_REPO_ROOT" || exit 9
export OUT="${OUT:-bench_out}"  # where the logs and results go (under the repository root)
mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1 TMPDIR=/tmp
: > $OUT/steps.log
step() {
    local name=$1 t=$2; shift 2
    local t0=$SECONDS
    timeout -k 10 "$t" "$@" > "$OUT/$name.log" 2>&1
    local rc=$?
    echo "[$name] rc=$rc $((SECONDS - t0)) s" >> $OUT/steps.log
    if grep -q "illegal memory access\|Memory access fault\|HSA_STATUS_ERROR" "$OUT/$name.log"; then
        echo "fault in $name: stopping" >> $OUT/steps.log; exit 7; fi
    if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stopping after $name rc=$rc" >> $OUT/steps.log; exit $rc; fi
    return 0
}
step accuracy 300 python -u tools/accuracy_probe.py
step stage_error 600 python -u tools/stage_error.py --images 0,1,2 -o $OUT/stage_error.json
step layer_error 600 python -u tools/layer_error.py --image 0
if [ "${TESTS:-1}" = "1" ]; then
  step pytest_gpu 900 python -u -m pytest tests -m gpu -q -rf --timeout 300 --timeout-method thread
fi
if [ "${BENCH:-1}" = "1" ]; then
  step bench_driver 900 python -u bench.py --full --gpus 1 --steps 20 --warmup 5
fi
exit 0
