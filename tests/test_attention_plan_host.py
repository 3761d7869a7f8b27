"""CPU: which attention kernel a launch takes (csrc/attention_plan.h, the decision of attention.hip's launchers as pure host functions).

Every form of the attention kernel -- four or eight waves, whole-row or 8-byte stores -- gives the same bits by design, so no GPU test
can see a batch start going to another form; only speed changes, or, as with the ``ld_qk % 64`` rule, results once the wrong kernel
is reached.  tests/attention_plan_main.cpp is compiled with the host C++ compiler against the header alone and fed shapes on stdin:

* the shapes tests/test_attention_io_gpu.py relies on (its ``LENS`` and ``CASES``, read from that module) plan to the kernel its
  docstring names;
* one case on either side of every condition of the wave rule, the mean-length condition, the grid limit and the switches;
* the workload's own shapes.

The expected values were read out of the launcher of the commit before the plan was one function, by hand.
"""
import os
import shutil
import subprocess

import pytest

import test_attention_io_gpu as IO
import test_attention_parity_gpu as PARITY

HERE = os.path.dirname(os.path.abspath(__file__))
GRID_LIMIT = 0x7FFFFFFF


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attention_plan") / "attention_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "attention_plan_main.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        return [tuple(int(t) for t in o.split()) for o in out[:-1]]

    return run


def shape(head_dim, heads, n_seq, max_len, total_rows=0, ld_qk=None, ld_out=None, out_scales=0, aligned=1, waves=0, line_stores=-1):
    """one launch; by default the encoder's own strides: Q | K side by side, the context as wide as the heads"""
    H = heads * head_dim
    return (f"plan {head_dim} {heads} {n_seq} {max_len} {total_rows} {2 * H if ld_qk is None else ld_qk} {H if ld_out is None else ld_out} "
            f"{out_scales} {aligned} {waves} {line_stores}")


def waves_of(plan, lines):
    return [g[0] for g in plan(lines)]


# the four-wave / eight-wave rule by hand for the lengths of test_attention_io_gpu.py, each alone (max_len = its own length,
# B = ceil(n / 32) blocks: eight waves for B = 5..8)
ALONE_64 = {1: 4, 31: 4, 32: 4, 33: 4, 64: 4, 127: 4, 128: 4, 129: 8, 160: 8, 257: 4, 292: 4}


def test_the_shapes_the_gpu_io_test_relies_on(plan):
    assert sorted(ALONE_64) == sorted(IO.LENS)
    assert {(dh, pad, ldq) for _, dh, pad, ldq in IO.CASES} == {(64, 8, 64), (64, 4, 64), (64, 8, 24), (32, 8, 64), (32, 4, 64)}
    for _, dh, pad, ldq in IO.CASES:
        heads = 2
        H = heads * dh
        kw = dict(ld_qk=2 * H + ldq, ld_out=H + pad)
        n = len(IO.LENS)
        # the batch as the test launches it: max_len = its longest sequence (292: ten blocks), and once more with max_len 512 (sixteen)
        batch, wide = plan([shape(dh, heads, n, max(IO.LENS), **kw), shape(dh, heads, n, 512, **kw)])
        alone = plan([shape(dh, heads, 1, m, **kw) for m in IO.LENS])
        if dh == 32:
            want_batch, want_wide, want_alone = 4, 4, [4] * n
        elif ldq % 64:                   # K rows not 128 bytes apart: the four-wave kernel's second K piece would come from the wrong columns
            want_batch, want_wide, want_alone = 8, 8, [8] * n
        else:
            want_batch, want_wide, want_alone = 4, 8, [ALONE_64[m] for m in IO.LENS]
        assert (batch[0], wide[0], [a[0] for a in alone]) == (want_batch, want_wide, want_alone), (dh, pad, ldq)
        # ld_out = H + 8 keeps rows 16-byte aligned: whole-row stores; H + 4 does not: the 8-byte stores
        assert {g[1] for g in [batch, wide] + alone} == {1 if pad == 8 else 0}, (dh, pad, ldq)
        # the grid is exact: one workgroup per 32 * waves query rows of max_len, per (sequence, head)
        for g, m, s in [(batch, 292, n), (wide, 512, n)] + [(a, m, 1) for a, m in zip(alone, IO.LENS)]:
            assert g[2] == -(-m // (32 * g[0])) and g[3] == heads * s * g[2], (dh, pad, ldq, m)
    # the f16c planes (out_scales) and an output base off the 16-byte grid keep the 8-byte stores
    assert [g[1] for g in plan([shape(64, 2, 11, 292, ld_out=136), shape(64, 2, 11, 292, ld_out=136, out_scales=1),
                                shape(64, 2, 11, 292, ld_out=136, aligned=0)])] == [1, 0, 0]


def test_the_wave_rule_on_both_sides_of_every_condition(plan):
    # head_dim 64, total_rows unknown: eight waves for B = 5..8 and 13..16 of every 16 blocks
    rule = {128: 4, 129: 8, 256: 8, 257: 4, 384: 4, 385: 8, 512: 8, 513: 4}
    assert waves_of(plan, [shape(64, 16, 100, m) for m in rule]) == list(rule.values())
    # 32-wide heads: four waves whatever the length
    assert waves_of(plan, [shape(32, 16, 100, m) for m in rule]) == [4] * len(rule)
    # the mean length: eight waves only from 0.7 max_len on (n_seq 10, max_len 160: 1120 rows); an unknown total counts as uniform lengths
    assert waves_of(plan, [shape(64, 16, 10, 160, total_rows=t) for t in (1120, 1119, 0, -1)]) == [8, 4, 8, 8]
    # a K row stride that is no multiple of 128 bytes: eight waves for 64-wide heads, at lengths of the four-wave class too
    assert waves_of(plan, [shape(64, 16, 100, m, ld_qk=2048 + off) for m in (64, 292) for off in (0, 64, 24, 8)]) == [4, 4, 8, 8] * 2
    assert waves_of(plan, [shape(32, 16, 100, 292, ld_qk=1024 + 24)]) == [4]


def test_the_workloads_shapes(plan):
    # the headline rerank step: 292 tokens, 16 heads x 64, Q | K rows of 2048, rows padded to 296 per pair
    for n_seq in (1600, 800):
        assert plan([shape(64, 16, n_seq, 292, total_rows=n_seq * 296, ld_qk=2048, ld_out=1024)]) == [(4, 1, 3, 16 * n_seq * 3)]
    # the RoPE and ModernBERT encoders launch on the fused projection's rows (ld_qk = 3 H): 768 and 1024 wide, a 512-token window batch
    assert plan([shape(64, 12, 64, 512, total_rows=64 * 512, ld_qk=2304, ld_out=768),
                 shape(64, 16, 64, 512, total_rows=64 * 512, ld_qk=3072, ld_out=1024),
                 shape(64, 12, 64, 292, total_rows=64 * 296, ld_qk=2304, ld_out=768)]) == \
        [(8, 1, 2, 12 * 64 * 2), (8, 1, 2, 16 * 64 * 2), (4, 1, 3, 12 * 64 * 3)]
    # bge-small (32-wide heads, 12 of them)
    assert plan([shape(32, 12, 256, 160, total_rows=256 * 160)]) == [(4, 1, 2, 12 * 256 * 2)]


def test_the_grid_is_exact_and_its_limit_is_the_launchers(plan):
    # 16 heads, one query tile: 134 217 727 sequences are the last product within the grid limit, one more is the first beyond it
    # (the plan states the count; tt_attention_launch refuses it)
    below, above = plan([shape(64, 16, 134217727, 128), shape(64, 16, 134217728, 128)])
    assert below == (4, 1, 1, 16 * 134217727) and below[3] <= GRID_LIMIT
    assert above == (4, 1, 1, 16 * 134217728) and above[3] == GRID_LIMIT + 1
    # no rounding of (sequence, head) pairs up to eight: 3 heads x 5 sequences x 3 tiles
    assert plan([shape(64, 3, 5, 292)]) == [(4, 1, 3, 45)]
    # the largest max_len an int holds: 2^26 blocks, eight waves, 2^23 tiles -- the block and tile counts are computed in 64 bits
    assert plan([shape(64, 16, 1, 2147483647, total_rows=2147483647)]) == [(8, 1, 8388608, 16 * 8388608)]


def test_the_switches(plan):
    # waves = 4 or 8 overrides the rule -- but not the stride rule, and not for 32-wide heads; 5 is no switch value any more
    assert waves_of(plan, [shape(64, 16, 100, 160, waves=4), shape(64, 16, 100, 292, waves=8), shape(64, 16, 100, 292, waves=4, ld_qk=2072),
                           shape(32, 16, 100, 160, waves=8), shape(64, 16, 100, 160, waves=5), shape(64, 16, 100, 292, waves=5)]) == \
        [4, 8, 8, 4, 8, 4]
    # line_stores = 0 turns whole-row stores off; 1 cannot turn them on where the rows or the base are not 16-byte aligned
    assert [g[1] for g in plan([shape(64, 16, 100, 292, line_stores=0), shape(64, 16, 100, 292, line_stores=1),
                                shape(64, 16, 100, 292, line_stores=1, ld_out=1028), shape(64, 16, 100, 292, line_stores=1, aligned=0),
                                shape(64, 16, 100, 292, line_stores=1, out_scales=1)])] == [0, 1, 0, 0, 0]


def test_the_cls_score_buffer(plan):
    limit = PARITY.CLS_LDS_LIMIT
    assert limit == 40953
    fits, over, one, most = plan([f"cls {limit}", f"cls {limit + 1}", "cls 1", "cls 2147483647"])
    assert most[0] == (2147483647 + 14) // 8 * 8 * 4
    assert fits[0] == 160 * 1024 and over[0] > 160 * 1024 and one[0] == 32

