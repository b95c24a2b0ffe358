"""CPU: what the 12 video doors keep apart and what they share, now that one check-and-launch path serves them all.  Every entry point and size
export is declared in include/ppms.h, exported, and bound with the header's argument list; the structs have the header's sizes, fields and offsets.  The 4:2:0 entry points accept
shift up to 20, the generic ones up to 26 - depth; and whatever is wrong with a call that is not about the maps, a plain entry point and its
_remap twin refuse it with one code and one message (ingest_util.one_message; the packed doors' cases of the same rule run in
tests/test_ingest_packed.py).  Table-driven from the BAD lists of the door's own test files.  No device."""
import ctypes

import pytest

import test_ingest_raw as RAW
import test_ingest_u8 as U8
import test_ingest_yuv as YUV420
import test_ingest_yuv_deep as YUV
from ingest_util import ENTRY_ARGS, FIELDS, SIZE_EXPORTS, ctype_of, header_args, lib, not_about_the_maps, one_message, refused, sized_maps  # noqa: F401  (lib: the fixture)

BYTES_420 = dict(fmt=dict(YUV.BYTES, sub_x=1, sub_y=1), left=dict(step_c=2), right=dict(step_c=2))        # the format the 4:2:0 entry points read
IDENTITY = dict(lmap={}, rmap={})                                                                         # (maps of the frames' own 37 x 50)


@pytest.mark.parametrize("name", [*ENTRY_ARGS, *SIZE_EXPORTS])
def test_declared_exported_and_bound_as_the_header_says_and_abi_version_unchanged(lib, name):
    from ppmstereo_amd import _lib as L
    args = header_args(name)
    assert args == (ENTRY_ARGS[name] if name in ENTRY_ARGS else SIZE_EXPORTS[name][0])
    assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.ppms_version() == 4
    res, bound = L._SIGS[name]
    assert res is ctypes.c_int and bound == [ctype_of(a) for a in args]
    if name in SIZE_EXPORTS:
        _, structs, sizes = SIZE_EXPORTS[name]
        said = [ctypes.c_int() for _ in structs]
        assert getattr(lib, name)(*(ctypes.byref(x) for x in said)) == 0
        assert tuple(x.value for x in said) == tuple(ctypes.sizeof(getattr(L, t)) for t in structs) == sizes
        assert getattr(lib, name)(*(None for _ in structs)) == 0
        for t in structs:                                           # the fields, in the header's order
            fields, offsets = FIELDS[t]
            assert [n for n, _ in getattr(L, t)._fields_] == fields
            assert {n: getattr(getattr(L, t), n).offset for n in offsets} == offsets


@pytest.mark.parametrize("twin", [False, True], ids=["plain", "remap"])
def test_the_two_shift_contracts(lib, twin):
    """shift = 20 passes the 4:2:0 entry's check of shift -- the later check of H fires; the generic entry at {1, 8, 0, 1, 1} stops at 26 - 8."""
    msg = refused(lib, YUV420._call(lib, twin=twin, shift=20, H=62), "yuv420_remap" if twin else "yuv420", "H = 62")
    assert b"shift" not in msg
    refused(lib, YUV420._call(lib, twin=twin, shift=21), "shift = 21", "[8, 20]")
    refused(lib, YUV._call(lib, shift=19, **BYTES_420, **(IDENTITY if twin else {})), "video_ingest_yuv_remap" if twin else "video_ingest_yuv:", "shift = 19", "[8, 18]")
    refused(lib, YUV._call(lib, shift=18, fnet=False, cnet=False, **BYTES_420, **(IDENTITY if twin else {})), "skipped")


# door: (the plain call, the same call through the _remap twin with maps whose source frame is the call's H0 x W0, the cases)
DOORS = {"u8": (U8._call, lambda lib, **bad: U8._call(lib, twin=True, **bad),
                U8.test_bad_arguments_return_einval_with_a_message_and_no_device.pytestmark[0].args[1]),
         "yuv420": (YUV420._call, lambda lib, **bad: YUV420._call(lib, twin=True, **bad), [b for _, b in YUV420.BAD]),
         "yuv": (YUV._call, lambda lib, **bad: YUV._call(lib, **bad, **sized_maps(bad)), [b for _, b in YUV.BAD]),
         "raw": (RAW._call, lambda lib, **bad: RAW._call(lib, **bad, **sized_maps(bad)), [b for _, b in RAW.BAD])}
# (the packed doors' cases run under the same rule in tests/test_ingest_packed.py, where their ids are)
PARITY = [(door, bad) for door, (_, _, cases) in DOORS.items() for bad in cases if not_about_the_maps(bad)]


@pytest.mark.parametrize("door,bad", PARITY, ids=[f"{d}:{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, (d, b) in enumerate(PARITY)])
def test_plain_entry_and_remap_twin_refuse_with_one_message(lib, door, bad):
    plain, twin, _ = DOORS[door]
    one_message(lib, door, plain, twin, bad)
