#!/bin/bash
# round 6: first-contact safety on the round-6 tree -- the two new / changed GPU tests and the two-rank RCCL-refusal fallback
# (eight ranks sharing one GPU are more processes than a shared device may have open: the 8-rank launch needs 8 GPUs)
cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p gpurun_out
timeout 1700 python -m pytest tests/test_two_ranks_gpu.py tests/test_pipeline_gpu.py tests/test_config5_gpu.py -m gpu -x -q 2>&1 | tail -8
