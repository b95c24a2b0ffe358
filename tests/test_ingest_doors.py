"""CPU: what the 8 video doors keep apart and what they share, now that one check-and-launch path serves them all.  The 4:2:0 entry points accept
shift up to 20, the generic ones up to 26 - depth; and whatever is wrong with a call that is not about the maps, a plain entry point and its
_remap twin refuse it with one code and one message.  Table-driven from the BAD lists of the door's own test files.  No device."""
import re

import pytest

import test_ingest_raw as RAW
import test_ingest_u8 as U8
import test_ingest_yuv as YUV420
import test_ingest_yuv_deep as YUV
from ingest_util import EINVAL, lib, refused  # noqa: F401  (lib: the fixture)

BYTES_420 = dict(fmt=dict(YUV.BYTES, sub_x=1, sub_y=1), left=dict(step_c=2), right=dict(step_c=2))        # the format the 4:2:0 entry points read
IDENTITY = dict(lmap={}, rmap={})                                                                         # (maps of the frames' own 37 x 50)


@pytest.mark.parametrize("twin", [False, True], ids=["plain", "remap"])
def test_the_two_shift_contracts(lib, twin):
    """shift = 20 passes the 4:2:0 entry's check of shift -- the later check of H fires; the generic entry at {1, 8, 0, 1, 1} stops at 26 - 8."""
    msg = refused(lib, YUV420._call(lib, twin=twin, shift=20, H=62), "yuv420_remap" if twin else "yuv420", "H = 62")
    assert b"shift" not in msg
    refused(lib, YUV420._call(lib, twin=twin, shift=21), "shift = 21", "[8, 20]")
    refused(lib, YUV._call(lib, shift=19, **BYTES_420, **(IDENTITY if twin else {})), "video_ingest_yuv_remap" if twin else "video_ingest_yuv:", "shift = 19", "[8, 18]")
    refused(lib, YUV._call(lib, shift=18, fnet=False, cnet=False, **BYTES_420, **(IDENTITY if twin else {})), "skipped")


def _sized_maps(bad):
    m = dict(hs=bad.get("H0", 37), ws=bad.get("W0", 50))
    return dict(lmap=m, rmap=m)


# door: (the plain call, the same call through the _remap twin with maps whose source frame is the call's H0 x W0, the cases)
DOORS = {"u8": (U8._call, lambda lib, **bad: U8._call(lib, twin=True, **bad),
                U8.test_bad_arguments_return_einval_with_a_message_and_no_device.pytestmark[0].args[1]),
         "yuv420": (YUV420._call, lambda lib, **bad: YUV420._call(lib, twin=True, **bad), [b for _, b in YUV420.BAD]),
         "yuv": (YUV._call, lambda lib, **bad: YUV._call(lib, **bad, **_sized_maps(bad)), [b for _, b in YUV.BAD]),
         "raw": (RAW._call, lambda lib, **bad: RAW._call(lib, **bad, **_sized_maps(bad)), [b for _, b in RAW.BAD])}
# not about the maps: the case names none, and its frame is one a map can name as its source frame (hs, ws >= 1)
PARITY = [(door, bad) for door, (_, _, cases) in DOORS.items() for bad in cases
          if not {"lmap", "rmap", "null_rmap"} & set(bad) and bad.get("H0", 1) >= 1 and bad.get("W0", 1) >= 1]


@pytest.mark.parametrize("door,bad", PARITY, ids=[f"{d}:{i}:" + ",".join(f"{k}={v}" for k, v in b.items()) for i, (d, b) in enumerate(PARITY)])
def test_plain_entry_and_remap_twin_refuse_with_one_message(lib, door, bad):
    plain, twin, _ = DOORS[door]
    said = []
    for entry in (plain, twin):
        lib.ppms_mem_attn_splits(3, 3, 256, 1)                  # (a successful call in between: the message below is this call's)
        assert entry(lib, **bad) == EINVAL, bad
        said.append(lib.ppms_last_error().decode())
    (name, text), (twin_name, twin_text) = (m.split(": ", 1) for m in said)
    assert twin_name == name + "_remap" and name == "video_ingest_" + door
    # the twin reads its frames' size from the maps and calls it hs x ws, the frames "source" frames: the only words that may differ
    assert re.sub(r"\bws\b", "W0", re.sub(r"\bhs\b", "H0", twin_text)).replace("a source frame's", "a frame's") == text, said
