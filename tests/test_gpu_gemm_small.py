"""The small GEMMs of csrc/gemm_f32.hip on the device, through the C ABI, against fp64 and exact integers at edge shapes (run with
-m gpu on an MI355X).  Cases, references and gates are gemm_ref.py's; test_gemm_ref.py proves on the CPU that the gates admit a
correct kernel and refuse a subtly wrong one.  Every case runs through BOTH tcar_gemm_f32_grouped (`gemm_f32_kernel`) and
tcar_gemm_x3_grouped (`gemm_x3_kernel`; the fused-epilogue fields dact / colsum / planes / pack are set for it alone), and through
tcar_gemm_f32 where it is one single-segment problem; a failure names the case, the entry point and the problem.

What a case holds: an integer case equals the int64 reference bit for bit (np.array_equal); a real-valued one stays inside the
forward bound (K + 4) 2^-24 G, plus 2^-16 G on the x3 kernel, and inside the project's `close`; planes and packed planes equal
bf16 hi / lo of the stored C at the KB32 offsets; every poisoned element around C, slabs, planes, packs and colsum is untouched, and
no NaN of the operand padding (columns past M / N / K, rows past the logical count) reaches a stored element.

What the table reaches (asserted on the CPU from the restated launcher arithmetic): both fp32 tiles in the three layouts, the
switch at 191 | 192 tiles of 128 x 128 with a one-element atomic ballast problem; M, N in {1, 3, 63, 64, 65, 129, 130} with tight
and wide leading dimensions; x3 stage counts 1 .. 6 with K tails of 4 .. 60, the ring switch at 4 | 5 stages, launches whose
problems disagree on the ring; 1 .. 3 segments of unequal K; 10-problem groups with empty problems in the middle and workgroup
counts that are no multiple of 8; split K with requested > effective counts, the collapse to one chunk, slabs folded by
tcar_splitk_reduce, atomics into a C that holds values; dact 1 / 2 with and without colsum, planes at a column offset, the packed
pair with a gap inside / empty / covering everything, bias + activation + planes, beta.

TcarOpt::hi_only and the completion flag are not reachable through the C ABI; they stay with the step-level tests.

Worst error / bound per group of real-valued cases, fp32 kernel | x3 kernel (the integer cases are exact on both):

    group       MI355X             numpy stand-in (CPU)
    edge        0.16 | 0.70        0.16 | 0.70        (x3: 0.70 at K = 16, 0.42 at 28, 0.36 at 36, 0.07 at 260)
    single      0.13 | 0.31        0.13 | 0.31
    tile128     0.10 | 0.39        0.12 | 0.39
    segments    0.02 | 0.08        0.02 | 0.08
    groups      0.12 | 0.41        0.14 | 0.41
    splitk      0.11 | 0.34        0.11 | 0.34
    epilogue    0.10 | 0.35        0.11 | 0.35
The x3 figures agree because products of bf16 values are exact in fp32: device and stand-in differ in the order of fp32 sums only.
The device tanhf stayed inside the 4 * 2^-24 the gate grants it.  401 tests, 3.4 s.
"""
import functools

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401
import gemm_ref as R
from gpu_util import lib, ptr  # noqa: F401  (lib: the module-scoped fixture)

pytestmark = pytest.mark.gpu

CASES = R.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
RUNS = [(c["name"], e) for c in CASES for e in R.entries(c)]


@functools.lru_cache(maxsize=2)
def built(name):
    """drawn once per case, shared by its entry points and never modified"""
    return R.build(BY_NAME[name])


@pytest.mark.parametrize("name,entry", RUNS)
def test_small_gemm(lib, name, entry):
    case = BY_NAME[name]
    w = R.check(case, built(name), R.run_device(lib, case, built(name), entry), entry)
    print("%-34s %-22s %-8s worst err / bound %.3f" % (name, entry, case["group"], w))


@pytest.mark.parametrize("M,N,S", [(1, 4, 3), (65, 68, 1), (1025, 2048, 2)])
def test_splitk_reduce_alone(lib, M, N, S):
    """tcar_splitk_reduce by itself on integers (exact in any order): one float4, one slab, and M N / 4 = 524,800 float4 — past
    the 2,048 blocks x 256 threads of its grid cap, so the grid-stride loop takes a second round"""
    assert (M * N // 4 > 2048 * 256) == (M == 1025)
    rng = np.random.RandomState(M + N)
    ld = N + 4
    slabs = np.full((S * M + 1, ld), np.nan, dtype=np.float32)
    slabs[:S * M, :N] = rng.randint(-8, 9, size=(S * M, N))
    out0 = np.full((M + 1, ld), R.SENT, dtype=np.float32)
    ds, do = torch.from_numpy(slabs).cuda(), torch.from_numpy(out0).cuda()
    assert lib.tcar_splitk_reduce(ptr(ds), S, M, N, ld, ptr(do), None) == 0
    torch.cuda.synchronize()
    got = do.cpu().numpy()
    want = out0.copy()
    want[:M, :N] = slabs[:S * M, :N].reshape(S, M, N).astype(np.int64).sum(0)
    assert np.array_equal(got, want)
