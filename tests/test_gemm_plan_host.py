"""CPU: which kernel a GEMM launch takes (csrc/gemm_plan.h, the decision of gemm.hip's launchers as a pure host function).

Every GEMM kernel form gives the same bits by design, so no GPU test can see a shape start going to another kernel -- only speed
changes.  tests/gemm_plan_main.cpp is compiled with the host C++ compiler against the header alone and fed shapes on stdin:

* every (kernel, shape) pair the GPU edge tests name (tests/test_gemm_edges_gpu.py, tests/test_gemm_x3_edges_gpu.py and their
  ``*_refs.py`` tables, read from those modules) plans to the kernel its label names on the 256 CUs of an MI355X;
* the workload's own shapes plan as they did before the plan was one function: the expected kernels and grids below were read out
  of the launchers of the commit before (``launch<EPI>``, ``launch_x3``, ``launch_fp8``, the QKV split) by hand, at 256 CUs and
  the default super-tile width 4, and confirmed by a kernel trace on the GPU (profiles/gemm_prune_ab.log);
* one case on either side of every condition of the rule.
"""
import os
import shutil
import subprocess

import pytest

import mid_refs as R
import test_gemm_edges_gpu as E16
import test_gemm_x3_edges_gpu as EX3
import x3_refs as X

HERE = os.path.dirname(os.path.abspath(__file__))
CUS = 256
BIAS, GELU, RES, TANH, QKV, VT, RELU = 0, 1, 2, 3, 4, 5, 7
LABEL = {"skinny": "Skinny", "relay": "Relay", "staged": "Staged128", "twostage": "TwoStage128", "onetile": "OneTile256",
         "tile256": "OneTile256", "persistent": "Persistent256"}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "gemm_plan_main.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        return [tuple(int(t) if t.lstrip("-").isdigit() else t for t in o.split()) for o in out[:-1]]

    return run


def b16(epi, M, N, K, cus=CUS):
    """tt_gemm_bf16 / tt_gemm_f16: lda = K, ldc = ldr = N"""
    return f"16 {epi} {M} {N} {K} {K} {N} {N} {cus}"


def x3(epi, M, N, K, cus=CUS):
    """planes [.][2K]; planes output [M][2N]"""
    return f"x3 {epi} {M} {N} {K} {2 * K} {2 * N} {2 * N} {cus}"


def _table(test_fn, names):
    for m in test_fn.pytestmark:
        if m.name == "parametrize" and m.args[0] == names:
            return list(m.args[1])
    raise AssertionError(f"{test_fn.__name__} has no table {names}")


def test_every_labelled_shape_of_the_gpu_edge_tests_reaches_the_kernel_it_names(plan):
    cases = []            # (label, input line)
    for kernel, (M, N, K) in E16.GEMM_PARAMS + _table(E16.test_gemm_operands_at_offsets, "kernel,shape"):
        cases += [(kernel, b16(epi, M, N, K)) for epi in R.gemm_epis(kernel)]
    for kernel, epi in _table(E16.test_epilogue_sweep, "kernel,epi"):
        cases.append((kernel, b16(epi, *R.SWEEP_SHAPES[kernel])))
    for kernel, shape in _table(E16.test_fp16_saturates_behind_the_residual_and_the_gelu, "kernel,shape"):
        cases.append((kernel, b16(RES, *shape)))
    x3_shapes = X.PARAMS + _table(EX3.test_the_forwards_own_layouts, "kernel,shape")
    x3_shapes += [(k, (rows, *X.IDENTITY_NK)) for k, rows in X.IDENTITY_ROWS.items()] + list(X.SWEEP_SHAPES.items())
    for kernel, (M, N, K) in x3_shapes:
        cases += [(kernel, x3(epi, M, N, K)) for epi in (BIAS, GELU, RES, VT)]
    assert {k for k, _ in cases} == set(LABEL), "a kernel label without a shape"
    got = plan([line for _, line in cases])
    wrong = [(k, line, g) for (k, line), g in zip(cases, got) if g[0] != LABEL[k]]
    assert not wrong, wrong


# (input line, (kernel, grid x, grid y)) -- 256 CUs, super-tile width 4; M = 473 600 = 1850 and 236 800 = 925 row tiles of 256
WORKLOAD = [
    # the headline step: Q | K columns and the V columns of the QKV projection (two launches), attention output, FFN up, FFN down
    (b16(BIAS, 473600, 2048, 1024), ("OneTile256", 14848, 1)), (b16(VT, 473600, 1024, 1024), ("OneTile256", 7424, 1)),
    (b16(RES, 473600, 1024, 1024), ("OneTile256", 7424, 1)), (b16(GELU, 473600, 4096, 1024), ("Persistent256", 256, 1)),
    (b16(RES, 473600, 1024, 4096), ("OneTile256", 7424, 1)),
    (b16(BIAS, 236800, 2048, 1024), ("OneTile256", 7424, 1)), (b16(VT, 236800, 1024, 1024), ("OneTile256", 3712, 1)),
    (b16(RES, 236800, 1024, 1024), ("OneTile256", 3712, 1)), (b16(GELU, 236800, 4096, 1024), ("Persistent256", 256, 1)),
    (b16(RES, 236800, 1024, 4096), ("OneTile256", 3712, 1)),
    (f"fp8 {GELU} 473600 4096 1024 1024 4096 4096 {CUS}", ("OneTile256", 29696, 1)),
    (f"fp8 {BIAS} 236800 2048 1024 1024 2048 2048 {CUS}", ("OneTile256", 7424, 1)),
    # a lone caller: one query (64 rows), a CLS tail (256), 10-20 reranked pairs (768, 3072, 7424 rows)
    (b16(BIAS, 64, 1024, 1024), ("Skinny", 64, 4)), (b16(GELU, 256, 4096, 1024), ("Skinny", 256, 16)),
    (b16(QKV, 64, 3072, 1024), ("Skinny", 192, 4)), (x3(BIAS, 64, 1024, 1024), ("Relay", 64, 4)),
    (x3(RES, 256, 1024, 4096), ("Relay", 64, 16)),
    (b16(QKV, 768, 3072, 1024), ("Staged128", 192, 1)), (b16(RES, 768, 1024, 1024), ("Staged128", 64, 1)),
    (b16(BIAS, 768, 1024, 1024), ("Staged128", 64, 1)),
    (b16(GELU, 768, 4096, 1024), ("Staged128", 256, 1)), (b16(RES, 768, 1024, 4096), ("Staged128", 64, 1)),
    (b16(BIAS, 3072, 2048, 1024), ("TwoStage128", 384, 1)), (b16(VT, 3072, 1024, 1024), ("OneTile256", 64, 1)),
    (b16(RES, 3072, 1024, 1024), ("Staged128", 192, 1)), (b16(GELU, 3072, 4096, 1024), ("OneTile256", 256, 1)),
    (b16(RES, 3072, 1024, 4096), ("Staged128", 192, 1)),
    (b16(BIAS, 7424, 2048, 1024), ("OneTile256", 256, 1)), (b16(VT, 7424, 1024, 1024), ("OneTile256", 128, 1)),
    (b16(RES, 7424, 1024, 1024), ("TwoStage128", 512, 1)), (b16(GELU, 7424, 4096, 1024), ("Persistent256", 256, 1)),
    (b16(RES, 7424, 1024, 4096), ("TwoStage128", 512, 1)),
    (x3(BIAS, 768, 1024, 1024), ("Staged128", 64, 1)), (x3(BIAS, 768, 3072, 1024), ("Staged128", 192, 1)),
    (x3(GELU, 768, 4096, 1024), ("Staged128", 256, 1)), (x3(RES, 768, 1024, 4096), ("Staged128", 64, 1)),
    (x3(RES, 3072, 1024, 1024), ("Staged128", 192, 1)), (x3(BIAS, 3072, 3072, 1024), ("OneTile256", 192, 1)),
    (x3(GELU, 3072, 4096, 1024), ("OneTile256", 256, 1)), (x3(RES, 3072, 1024, 4096), ("Staged128", 192, 1)),
    (x3(RES, 7424, 1024, 1024), ("Staged128", 512, 1)), (x3(GELU, 7424, 4096, 1024), ("OneTile256", 512, 1)),
    (x3(RES, 7424, 1024, 4096), ("Staged128", 512, 1)),
    # bge-small (hidden 384 = 3 column tiles of 128) at 4096 rows
    (b16(RES, 4096, 384, 384), ("Staged128", 96, 1)), (b16(QKV, 4096, 1152, 384), ("TwoStage128", 512, 1)),
    (b16(GELU, 4096, 1536, 384), ("TwoStage128", 512, 1)), (b16(RES, 4096, 384, 1536), ("Staged128", 96, 1)),
    (x3(RES, 4096, 384, 384), ("Staged128", 96, 1)), (x3(BIAS, 4096, 1152, 384), ("Staged128", 512, 1)),
    (x3(GELU, 4096, 1536, 384), ("Staged128", 512, 1)), (x3(RES, 4096, 384, 1536), ("Staged128", 96, 1)),
]


def test_the_workloads_shapes_plan_as_before(plan):
    got = plan([line for line, _ in WORKLOAD])
    wrong = [(line, want, g) for (line, want), g in zip(WORKLOAD, got) if g != want]
    assert not wrong, wrong
    # the QKV projection runs as two launches from 128 tiles of 256^2 on (ldc = 2 H for Q | K, ldvt = 8 H)
    assert plan([f"qkv {M} 3072 2048 2048 8192" for M in (473600, 236800, 7424, 3072, 768)] + ["qkv 4096 1152 768 768 3072"]) == \
        [(1,), (1,), (1,), (1,), (0,), (0,)]


# one case on either side of every condition
BOUNDARIES = [
    # up to 256 rows: the weight-streaming kernels (320 rows are refused by the launchers; whatever they plan, it is no skinny kernel)
    (b16(BIAS, 256, 1024, 1024), "Skinny"), (b16(BIAS, 320, 1024, 1024), "!Skinny"),
    (x3(BIAS, 256, 1024, 1024), "Relay"), (x3(BIAS, 320, 1024, 1024), "!Relay"), (x3(BIAS, 320, 1024, 1024), "!Skinny"),
    (b16(BIAS, 512, 1024, 1024), "Staged128"),
    # 127 and 128 tiles of 256^2: the small grid of 128^2 tiles below
    (b16(BIAS, 127 * 256, 256, 64), "TwoStage128"), (b16(BIAS, 128 * 256, 256, 64), "OneTile256"),
    # ... which the V^T epilogue has no form for
    (b16(VT, 512, 256, 64), "OneTile256"),
    # the persistent kernel (GELU): more workgroups than CUs (counted in eights) -- 256 blocks on 256 and on 248 CUs, 384 on 256
    (b16(GELU, 3072, 4096, 1024), ("OneTile256", 256, 1)), (b16(GELU, 3072, 4096, 1024, cus=248), ("Persistent256", 248, 1)),
    (b16(GELU, 4352, 4096, 1024), ("Persistent256", 256, 1)), (b16(GELU, 4352, 4096, 1024, cus=7), ("OneTile256", 384, 1)),
    (b16(BIAS, 4352, 4096, 1024), "OneTile256"), (b16(GELU, 32768, 256, 64), "OneTile256"),      # ... other epilogue; one K-tile
    # the staged 128^2 kernel, 16-bit: one round -- 256 tiles on 256 CUs, 257 tiles
    (b16(BIAS, 256 * 128, 128, 64), ("Staged128", 256, 1)), (b16(BIAS, 257 * 128, 128, 64), ("TwoStage128", 264, 1)),
    (b16(BIAS, 256 * 128, 128, 64, cus=255), "TwoStage128"),
    # ... split planes: two rounds -- 512 tiles on 256 CUs; M is a multiple of 256, so the next count is 514; 512 tiles on 255 CUs
    (x3(BIAS, 512 * 128, 128, 128), ("Staged128", 512, 1)), (x3(BIAS, 514 * 128, 128, 128), ("OneTile256", 288, 1)),
    (x3(BIAS, 512 * 128, 128, 128, cus=255), "OneTile256"),
    # the residual epilogue of the 256^2 kernels needs an even number of K-steps
    (b16(RES, 4096, 2048, 192), "TwoStage128"), (b16(BIAS, 4096, 2048, 192), "OneTile256"), (b16(RES, 4096, 2048, 128), "OneTile256"),
    # ... and 16-byte residual rows, like the output's
    (f"16 {RES} 4096 2048 128 128 2048 2052 {CUS}", "TwoStage128"), (f"16 {BIAS} 4096 2048 128 128 2052 2048 {CUS}", "TwoStage128"),
    # split planes: the staged kernel has whole 128-column tiles only
    (x3(BIAS, 512, 192, 128), "OneTile256"), (x3(BIAS, 512, 128, 128), "Staged128"),
]


def test_each_condition_of_the_rule_on_either_side(plan):
    got = plan([line for line, _ in BOUNDARIES])
    for (line, want), g in zip(BOUNDARIES, got):
        if isinstance(want, tuple):
            assert g == want, (line, want, g)
        elif want.startswith("!"):
            assert g[0] != want[1:], (line, want, g)
        else:
            assert g[0] == want, (line, want, g)
