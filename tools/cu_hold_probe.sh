cd ${GRAFT_REPO_ROOT:-.}
mkdir -p gpurun_out/r3r
timeout -k 10 600 python -m pytest tests/test_kernels_gpu.py tests/test_round2_gpu.py tests/test_round3_gpu.py -q -m gpu -x -k "gemm or wgrad or headline or block" > gpurun_out/r3r/tests.log 2>&1; echo "tests rc=$?"; tail -2 gpurun_out/r3r/tests.log
timeout -k 10 300 python tools/cu_hold_probe.py 2>&1 | grep -v Warning
