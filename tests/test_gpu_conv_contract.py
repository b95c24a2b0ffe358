"""GPU: rated means accepted and correct.  Wherever a rating function of the library answers non-zero for a descriptor, the matching launch entry
point takes it (called as convplan.ConvOp calls it: the library's own hints, the rated slice count) and the result agrees with the float64
reference of tests/conv_audit.py at the conv tests' bound (3e-5 * max(1, |ref|max)).  Where the rating is 0 nothing is launched."""
import ctypes as C
import math

import pytest
import torch

import conv_audit as A
from ppmstereo_amd import _lib as L
from ppmstereo_amd.convplan import CONV2, CONV2_SWEPT, CONV5, CONV6, GEMM1, STREAM, ConvOp, epilogue, pack_for
from ppmstereo_amd.weights import hash_normal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SMALL = [(1, 5, 7), (2, 8, 32), (3, 23, 40)]
LARGE = [(5, 80, 128)]        # the smallest map of the existing tests on which conv_gemm5 and conv_gemm6 rate non-zero at 256 CUs (>= 200 tiles)
MS = [64, 128, 192, 256]
TAPS = [(1, 1, 1), (1, 1, 5), (1, 5, 1), (1, 3, 3), (5, 1, 1), (3, 3, 3)]
SEGS = [[128], [128, 256]]

# form -> (kernel, pack key, maps, rating(lib, d) -> (served, nslice), ConvOp keywords)
FORMS = {
    "conv_gemm2": (CONV2, CONV2, SMALL, lambda lib, d: (lib.ppms_conv_gemm2_slices(d) == 1, 1), {}),
    "conv_gemm2_sliced": (CONV2, CONV2, SMALL, lambda lib, d: (lib.ppms_conv_gemm2_slices(d) > 1, lib.ppms_conv_gemm2_slices(d)), {}),
    "conv_gemm2_ysweep": (CONV2, CONV2_SWEPT, SMALL, lambda lib, d: (lib.ppms_conv_gemm2_ysweep_slices(d) > 0, max(1, lib.ppms_conv_gemm2_ysweep_slices(d))),
                          dict(ysweep=True)),
    "gemm1": (GEMM1, GEMM1, SMALL, lambda lib, d: (lib.ppms_gemm1_applicable(d) != 0, 1), {}),
    "conv_stream": (STREAM, STREAM, SMALL, lambda lib, d: (lib.ppms_conv_stream_applicable(d) != 0, 1), {}),
    "conv_gemm5": (CONV5, CONV5, LARGE, lambda lib, d: (lib.ppms_conv_gemm5_applicable(d) != 0, 1), {}),
    "conv_gemm6": (CONV6, CONV6, LARGE, lambda lib, d: (lib.ppms_conv_gemm6_applicable(d) != 0, 1), {}),
}


def _servable_pack(kernel, M, k3, segs):
    """Whether packing.py has a layout of this kernel for the shape at all (no pack: the planner never asks the rating)."""
    if kernel in (CONV5, CONV6):
        return M in (128, 192, 256)
    if kernel == GEMM1:
        return k3 == (1, 1, 1)
    return True


@pytest.mark.parametrize("form", list(FORMS))
def test_rated_means_accepted_and_correct(form):
    assert torch.cuda.is_available(), "these tests need the MI355X (no CPU fallback exists)"
    lib = L.load()
    kernel, pack_key, maps, rate, kw = FORMS[form]
    launched = 0
    for T, H, W in maps:
        P = T * H * W
        xin = {c: L.SPTensor(P, c, DEV) for c in (128, 256)}
        out = L.SPTensor(P, 256, DEV)
        for segs in SEGS:
            for k3 in TAPS:
                cin = sum(segs)
                for M in MS:
                    if not _servable_pack(pack_key, M, k3, segs):
                        continue
                    wt = hash_normal((M, cin, *k3), 7000 + M + cin) / math.sqrt(cin * k3[0] * k3[1] * k3[2])
                    packed, bias, meta = pack_for(pack_key, wt.to(DEV), (hash_normal((M,), 7001) * 0.1).to(DEV), segs, segs, None, M)
                    assert meta["M"] == M
                    d = L.Conv()
                    for i, c in enumerate(segs):
                        d.seg[i] = xin[c].view()
                    d.nseg, d.w, d.bias = len(segs), packed.data_ptr(), bias.data_ptr()
                    d.T, d.H, d.W = T, H, W
                    d.kt, d.kh, d.kw = k3
                    d.M = d.m_split = M
                    d.epi[0] = epilogue(n_valid=M, out_sp=out.view(0, M))
                    served, nslice = rate(lib, C.byref(d))
                    if not served:
                        continue                                   # rating 0: nothing is launched
                    keep = [xin[c] for c in segs] + [packed, bias, out]
                    op = ConvOp(d, keep, kernel, nslice=nslice, **kw)
                    assert op.nslice == nslice
                    pool = A.Pool(keep)
                    rs, errs = A.bind_regions(d, pool)
                    assert not errs, (form, (T, H, W), segs, k3, M, errs)
                    A.fill_storages(pool, rs, d, seed=M + k3[0] + 3 * k3[1] + 7 * k3[2])
                    pix = A.pixel_sample(T, H, W, 0, A.pix_device(pool))
                    exp = A.reference(d, op.version, op.ysweep, pool, rs, pix)
                    op()                                           # the call must succeed (L.check raises on a refusal)
                    torch.cuda.synchronize()
                    fails, _ = A.compare(exp, A.got_values(d, pool, rs, pix), d)
                    assert not fails, (form, (T, H, W), segs, k3, M, nslice, fails)
                    launched += 1
    assert launched >= 3, f"{form}: only {launched} of the cases are rated -- the test would pass by skipping everything"
