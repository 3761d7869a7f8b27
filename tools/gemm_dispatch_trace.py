"""Which kernel each GEMM shape of the workload is dispatched to, from a kernel trace (the check beside tests/test_gemm_plan_host.py).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/gemm_dispatch_trace.py      one launch per shape
    python tools/gemm_dispatch_trace.py --table OUT                                       the trace as a table: shape, kernel, workgroups

Shapes: the headline step's four projections at M = 473 600 and 236 800 (16-bit and e4m3), a lone caller's at M = 64, 256, 768,
3072 and 7424 (16-bit and split planes) and bge-small's at M = 4096.  Operands are zeros: only the dispatch is looked at.
TT_LIB_NAME names the library, as everywhere.
"""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIAS, GELU, RES = 0, 1, 2
LAYER = [(3072, 1024, BIAS), (1024, 1024, RES), (4096, 1024, GELU), (1024, 4096, RES)]
SMALL = [(384, 384, RES), (1152, 384, BIAS), (1536, 384, GELU), (384, 1536, RES)]


def calls():
    """(form, M, N, K, epilogue) in launch order"""
    out = [("16", M, n, k, e) for M in (473600, 236800) for n, k, e in LAYER]
    out += [("fp8", M, n, k, e) for M in (473600, 236800) for n, k, e in LAYER if e != RES]
    for M in (64, 256, 768, 3072, 7424):
        out += [(form, M, n, k, e) for form in ("16", "x3") for n, k, e in LAYER]
    out += [(form, 4096, n, k, e) for form in ("16", "x3") for n, k, e in SMALL]
    return out


def launch_all():
    import torch

    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    z = lambda *shape, dtype=torch.bfloat16: torch.zeros(shape, dtype=dtype, device=dev)
    for form, M, N, K, epi in calls():
        bias = z(N, dtype=torch.float32)
        if form == "16":
            a, w, c, r = z(M, K), z(N, K), z(M, N), z(M, N)
            rc = lib.tt_gemm_bf16(a.data_ptr(), w.data_ptr(), bias.data_ptr(), r.data_ptr() if epi == RES else None, c.data_ptr(), M, N, K, epi, st)
        elif form == "fp8":
            a, w, c = z(M, K, dtype=torch.uint8), z(N, K, dtype=torch.uint8), z(M, N)
            sa, sw = z(M, dtype=torch.float32), z(N, dtype=torch.float32)
            rc = lib.tt_gemm_fp8(a.data_ptr(), sa.data_ptr(), w.data_ptr(), sw.data_ptr(), bias.data_ptr(), c.data_ptr(), M, N, K, epi, st)
        else:
            a, w, c, c32, r32 = z(M, 2 * K), z(N, 2 * K), z(M, 2 * N), z(M, N, dtype=torch.float32), z(M, N, dtype=torch.float32)
            # residual epilogue: fp32 out [M][ldc = N] = acc + bias + fp32 residual [M][ldr = N]; else planes out [M][ldc = 2N], lo at column N
            rc = lib.tt_gemm_x3_ex(a.data_ptr(), w.data_ptr(), bias.data_ptr(), r32.data_ptr() if epi == RES else None, None, N, 0,
                                   c.data_ptr(), N if epi == RES else 2 * N, N, c32.data_ptr(), None, None, 0, M, N, K, epi, st)
        torch.cuda.synchronize()
        assert rc == 0, (form, M, N, K, epi, rc, lib.tt_last_error())
    print(f"{len(calls())} GEMM launches [{os.environ.get('TT_LIB_NAME') or 'libtt_hip.so'}]")


def short(name):
    return re.sub(r"^void |\(anonymous namespace\)::|\(GemmParams(, int)?\)$", "", name)


def table(out_dir):
    paths = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, paths
    rows = [r for r in csv.DictReader(open(paths[0])) if "gemm_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(calls()), (len(rows), len(calls()))
    counts = {}
    for (form, M, N, K, epi), r in zip(calls(), rows):
        k = short(r["Kernel_Name"])
        counts[k] = counts.get(k, 0) + 1
        wgs = [int(r[f"Grid_Size_{d}"]) // max(1, int(r[f"Workgroup_Size_{d}"])) for d in "XY"]
        print(f"{form:>3} epi {epi} {M:>6} x {N:>4} x {K:>4}  {k:<52} workgroups {wgs[0]} x {wgs[1]}")
    print("-- launches per kernel")
    for k in sorted(counts):
        print(f"{counts[k]:>3}  {k}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        launch_all()
