"""CPU: the descriptor contract of the five convolution kernels (csrc/conv_check.h) -- the rating functions and the launch entry points
refuse the same descriptors, and a refusal names the kernel and the field.  Host code only: every check precedes the first HIP call, so a
refused launch touches no GPU (the pointers below are never dereferenced)."""
import ctypes as C

import pytest

from ppmstereo_amd import _lib as L

EINVAL = -1
DEV, WS = 0x6000, 0x70000000          # stand-ins for the device descriptor copy / the slice workspace of a launch that must be refused


def _desc(T, H, W, M, k3, seg_c):
    """As tests/test_host_logic.py::_desc: good enough for the host-side planners."""
    d = L.Conv()
    for i, c in enumerate(seg_c):
        d.seg[i] = L.SP(0x1000, 0x2000, c, c)
    d.nseg, d.w, d.bias = len(seg_c), 0x3000, 0x4000
    d.T, d.H, d.W = T, H, W
    d.kt, d.kh, d.kw = k3
    d.M = d.m_split = M
    d.epi[0].n_valid = M
    return d


def _forms():
    """name -> (kernel name in messages, a descriptor its rating accepts, [(rating, its 'not served' answer)], launch(lib, d, rating answer))."""
    lib = L.load()
    return {
        "conv_gemm2": ("conv_gemm2", lambda: _desc(5, 20, 32, 256, (1, 3, 1), [128]),
                       [(lib.ppms_conv_gemm2_ysweep_slices, 0), (lib.ppms_conv_gemm2_slices, 1)],
                       lambda d, n: lib.ppms_conv_gemm2_ysweep(C.byref(d), DEV, max(n, 1), WS, None)),
        "conv_gemm2_plain": ("conv_gemm2", lambda: _desc(5, 20, 32, 256, (1, 1, 15), [128, 384]), [(lib.ppms_conv_gemm2_slices, 1)],
                             lambda d, n: lib.ppms_conv_gemm2(C.byref(d), DEV, 0, None)),
        "conv_gemm5": ("conv_gemm5", lambda: _desc(5, 80, 128, 256, (1, 1, 5), [128, 256]), [(lib.ppms_conv_gemm5_applicable, 0)],
                       lambda d, n: lib.ppms_conv_gemm5(C.byref(d), DEV, 0, None)),
        "conv_gemm5_sliced": ("conv_gemm5", lambda: _desc(5, 40, 64, 128, (1, 1, 3), [256]), [(lib.ppms_conv_gemm5_slices, 0)],
                              lambda d, n: lib.ppms_conv_gemm5_sliced(C.byref(d), DEV, 0, max(n, 2), WS, None)),
        "conv_gemm6": ("conv_gemm6", lambda: _desc(5, 80, 128, 256, (1, 1, 5), [128, 256]), [(lib.ppms_conv_gemm6_applicable, 0)],
                       lambda d, n: lib.ppms_conv_gemm6(C.byref(d), DEV, None)),
        "gemm1": ("gemm1", lambda: _desc(5, 20, 32, 128, (1, 1, 1), [128]), [(lib.ppms_gemm1_applicable, 0)],
                  lambda d, n: lib.ppms_gemm1(C.byref(d), DEV, 0, None)),
        "conv_stream": ("conv_stream", lambda: _desc(5, 20, 32, 128, (1, 1, 5), [128, 384]), [(lib.ppms_conv_stream_applicable, 0)],
                        lambda d, n: lib.ppms_conv_stream(C.byref(d), DEV, 0, None)),
    }


FORMS = ["conv_gemm2", "conv_gemm2_plain", "conv_gemm5", "conv_gemm5_sliced", "conv_gemm6", "gemm1", "conv_stream"]
RATES_OPERANDS = {"gemm1", "conv_stream"}          # their ratings check the operand tier too (they always did)
NO_OUT_VT = {"conv_gemm6", "conv_stream", "conv_gemm5_sliced"}
NO_ADDF32 = {"gemm1", "conv_stream"}


def _set(**kw):
    def f(d, form):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


def _seg0(**kw):
    def f(d, form):
        for k, v in kw.items():
            setattr(d.seg[0], k, v(d.seg[0]) if callable(v) else v)
    return f


def _groups(d, form):
    d.groups = 3 if form == "conv_gemm6" else 2          # (conv_gemm6 serves two groups)


def _bad_m(d, form):
    d.M = d.m_split = d.epi[0].n_valid = 80


def _kind(d, form):
    d.epi[0].kind = L.EPI_ADDF32 if form in NO_ADDF32 else 9
    d.epi[0].out_f32, d.epi[0].out_f32_ld = 0x8000, d.M


def _out_vt(d, form):
    d.epi[0].out_vt = 0x5000


def _n_valid(d, form):
    d.epi[0].n_valid = 0


# field, tier, what breaks it, the text that names the field in the refusal
TABLE = [
    ("groups", "shape", _groups, "groups="),
    ("even tap", "shape", _set(kw=4), "kw=4"),
    ("t_halo", "shape", _set(t_halo=9), "t_halo=9"),
    ("misaligned plane", "shape", _seg0(hi=lambda s: s.hi + 4), "seg[0] planes not 16-B aligned"),
    ("ld", "shape", _seg0(ld=1028), "seg[0].ld=1028"),
    ("channel multiple", "shape", _seg0(c=8), "seg[0].c=8"),
    ("M", "shape", _bad_m, "M=80"),
    ("nseg", "shape", _set(nseg=3), "nseg=3"),
    ("w", "operand", _set(w=None), "w/bias missing"),
    ("n_valid", "operand", _n_valid, "epi[0].n_valid=0"),
    ("kind", "kind", _kind, "epi[0].kind="),
    ("out_vt", "shape", _out_vt, "out_vt"),
]


@pytest.mark.parametrize("form", FORMS)
def test_rating_and_launch_refuse_the_same_descriptors(form):
    """One field at a time broken in a descriptor the rating accepts: a shape-tier field makes every rating of the kernel answer 'not served';
    every field makes the launch entry point return PPMS_EINVAL with '<kernel>: <field>...' as the message.  The operand tier (w, bias, the
    epilogue's operands) is left to the launch by conv_gemm2 / 5 / 6, whose ratings keep their answer; gemm1 and conv_stream rate it too."""
    lib = L.load()
    kernel, good, ratings, launch = _forms()[form]
    base = [fn(C.byref(good())) for fn, _ in ratings]
    assert base[0] > 0, (form, base)
    for field, tier, breaker, text in TABLE:
        if field == "out_vt" and form not in NO_OUT_VT:
            continue                                       # served there
        if tier == "kind":
            tier = "shape" if form in NO_ADDF32 else "operand"
        d = good()
        breaker(d, form)
        got = [fn(C.byref(d)) for fn, _ in ratings]
        if tier == "shape" or form in RATES_OPERANDS:
            assert got == [ns for _, ns in ratings], (form, field, got)
        else:
            assert got == base, (form, field, got, base)
        assert launch(d, base[0]) == EINVAL, (form, field)
        msg = lib.ppms_last_error().decode()
        assert msg.startswith(kernel + ":") and text in msg, (form, field, msg)


def test_ratings_that_used_to_drift_from_their_launch():
    """The descriptors on a 5 x 80 x 128 map with M = 256 that ppms_conv_gemm5_applicable / ppms_conv_gemm6_applicable used to rate 1 although
    the launch entry point refuses them."""
    lib = L.load()
    r5, r6 = lib.ppms_conv_gemm5_applicable, lib.ppms_conv_gemm6_applicable
    l5 = lambda d: lib.ppms_conv_gemm5(C.byref(d), DEV, 0, None)
    l6 = lambda d: lib.ppms_conv_gemm6(C.byref(d), DEV, None)
    err = lambda: lib.ppms_last_error().decode()
    good = lambda k3=(1, 1, 5), segs=(128, 256): _desc(5, 80, 128, 256, k3, list(segs))
    assert r5(C.byref(good())) == 1 and r6(C.byref(good())) == 1

    d = good(segs=(128, 128))                              # grouped: conv_gemm6 only
    d.groups, d.m_split = 2, 128
    d.epi[0].n_valid = d.epi[1].n_valid = 128
    assert r5(C.byref(d)) == 0 and l5(d) == EINVAL and "grouped" in err()
    assert r6(C.byref(d)) == 1
    d = good((1, 1, 4))                                    # even taps
    assert r5(C.byref(d)) == 0 and l5(d) == EINVAL and "kw=4" in err()
    d = good((2, 1, 3))
    assert r5(C.byref(d)) == 0 and r6(C.byref(d)) == 0 and l5(d) == EINVAL and "kt=2" in err() and l6(d) == EINVAL and "kt=2" in err()
    d = good()                                             # a segment plane at a 4-byte offset
    d.seg[0].hi += 4
    assert r5(C.byref(d)) == 0 and r6(C.byref(d)) == 0 and l5(d) == EINVAL and "16-B aligned" in err() and l6(d) == EINVAL and "16-B aligned" in err()
    d = good()                                             # ld = 1028: not a multiple of 8 (and beyond conv_gemm6's 1024)
    d.seg[0].ld = 1028
    assert r6(C.byref(d)) == 0 and r5(C.byref(d)) == 0 and l6(d) == EINVAL and "seg[0].ld=1028" in err()
    d = good()
    d.seg[0].ld = d.seg[1].ld = 1032                       # a multiple of 8 beyond the cap: conv_gemm6 alone refuses
    assert r6(C.byref(d)) == 0 and l6(d) == EINVAL and "seg[0].ld=1032 (<= 1024)" in err() and r5(C.byref(d)) == 1
    d = good()
    d.t_halo = 9
    assert r5(C.byref(d)) == 0 and r6(C.byref(d)) == 0 and l5(d) == EINVAL and "t_halo=9" in err() and l6(d) == EINVAL and "t_halo=9" in err()


def test_ratings_do_not_look_at_the_operands():
    """ppms_conv_gemm5_applicable / ppms_conv_gemm6_applicable / the conv_gemm2 slice planners rate a descriptor before its weights and
    epilogue are filled in (convplan.plan_conv rates, then packs)."""
    lib = L.load()
    d = _desc(5, 80, 128, 256, (1, 3, 3), [128])
    d.w = d.bias = None
    d.epi[0].n_valid = 0
    assert lib.ppms_conv_gemm5_applicable(C.byref(d)) == 1 and lib.ppms_conv_gemm6_applicable(C.byref(d)) == 1
    d.T, d.H, d.W, d.kw = 5, 20, 32, 1
    assert lib.ppms_conv_gemm2_ysweep_slices(C.byref(d)) >= 1 and lib.ppms_conv_gemm5_slices(C.byref(d)) >= 2
