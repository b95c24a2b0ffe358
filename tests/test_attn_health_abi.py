"""CPU: the planner query and the fix-up accounting entry point of the memory attention are part of the C ABI (include/ppms.h), and
ppms_mem_attn_splits answers without a GPU.  No compute."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ppmstereo_amd import _lib as L
    return L.load()


@pytest.mark.parametrize("f", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("ksel", [1, 2, 3, 4, 5])
def test_splits_is_ceil_of_picked_frames_over_frames_per_workgroup(lib, ksel, f):
    for T in (1, 3, 5):
        assert lib.ppms_mem_attn_splits(T, ksel, 256, f) == -(-ksel // f)


def test_splits_is_zero_where_the_64_query_kernel_does_not_serve(lib):
    for f in range(6):
        assert lib.ppms_mem_attn_splits(3, 3, 200, f) == 0           # n % 64 != 0: the 32-query kernel runs, no redo flags exist


def test_splits_refuses_bad_arguments(lib):
    assert lib.ppms_mem_attn_splits(3, 0, 256, 1) < 0
    assert b"ksel=0" in lib.ppms_last_error()
    assert lib.ppms_mem_attn_splits(3, 6, 256, 1) < 0
    assert lib.ppms_mem_attn_splits(0, 3, 256, 1) < 0
    assert lib.ppms_mem_attn_splits(3, 3, 0, 1) < 0
    assert lib.ppms_mem_attn_splits(3, 3, 256, 6) < 0
    assert lib.ppms_mem_attn_splits(3, 3, 256, -1) < 0


def test_accumulate_refuses_bad_arguments_without_a_gpu(lib):
    assert lib.ppms_attn_redo_accumulate(None, 3, 3, 256, 1, None, None) < 0
    assert b"null" in lib.ppms_last_error()


def test_both_symbols_are_declared_and_bound(lib):
    from ppmstereo_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "ppms.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ppms_mem_attn_splits\s*\(\s*int T, int ksel, int n, int frames_per_workgroup\s*\)", src)
    assert re.search(r"\bint\s+ppms_attn_redo_accumulate\s*\(\s*const void\* split_ws, int T, int ksel, int n, int frames_per_workgroup, "
                     r"int64_t\* counters, void\* stream\s*\)", src)
    for name in ("ppms_mem_attn_splits", "ppms_attn_redo_accumulate"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.ppms_version() == 4


def test_engine_and_public_interface_signatures():
    import inspect

    from ppmstereo_amd.engine import ScaleEngine
    from ppmstereo_amd.ppmstereo import PPMStereo, PPMStereoHotPath
    for name in ("enable_attn_health", "attn_health", "reset_attn_health", "attn_redo_count"):
        assert callable(getattr(ScaleEngine, name))
    assert inspect.signature(ScaleEngine.enable_attn_health).parameters["on"].default is True
    assert inspect.signature(PPMStereoHotPath.cascade).parameters["diagnostics"].default is None
    assert inspect.signature(PPMStereo.forward).parameters["diagnostics"].default is None
    assert inspect.signature(PPMStereo.forward_batch_test).parameters["diagnostics"].default is False
