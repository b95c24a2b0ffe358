"""GPU: the colour plane crosses the streams.  It is allocated and written on the caller's stream, directly behind the ingest launch and in front of
both encoders; the coloured cloud's place launch reads it on the 1/4 scale's stream (``ClipPipeline.large``), and the device -> host copy on the
caller's again.  No event, stream or wait was added for it: the 1/4 scale is ordered behind the small scales, those behind the caller's stream, and
the plane is held by the call object and the result dict (and told to the allocator with record_stream on the stream that reads it).  The proof
is tests/test_gpu_stream_order.py's whole-call case with ``colour=`` and the "xyzrgb" cloud: the several-window forward_batch_test with each role
held back in turn (tests/stream_hold.py) gives the bytes of the unheld call.  A stream that is in no role raises UnknownStream there."""
import pytest
import torch

from egress_util import Q, RIG_CAL
from ppmstereo_amd.ppmstereo import OutputSpec
from test_gpu_stream_order import TAGS, VideoCase, held_run, model, timing, unheld  # noqa: F401  (model, timing: the fixtures)

pytestmark = pytest.mark.gpu

SPEC = OutputSpec(disparity="u16", uncertainty="u8", colour="bgra8", cloud="f32", cloud_layout="xyzrgb", cloud_index=True, Q=Q, max_uncertainty=0.5, **RIG_CAL)
# the roles of the whole call: the caller's stream, cnet's, the pipeline's two, every engine's side stream and the hoisted blocks' pre-activation streams
ROLES = ["caller", "enc.side", "pipe.small", "pipe.large"] + [f"side:{t}" for t in TAGS] + [f"pre:{t}" for t in TAGS[1:]]


class ColourVideoCase(VideoCase):
    """VideoCase (7 frames of 60 x 250 uint8, kernel_size = 4: two windows of 4 and 3 frames, a ClipPipeline) with the coloured output."""

    def run(self):
        with self.one_pipeline():
            out = self.model.forward_batch_test({"stereo_video": self.va}, kernel_size=4, iters=4, output=SPEC)
        torch.cuda.synchronize()
        return out

    def reference(self):
        if self.measured is None:
            self.measured = unheld("colour video", self.roles, self.run, self.prepare)
        return self.measured


_CASE = []


def flat(result):
    """The result's tensors in a fixed order: the planes, then every frame's records and indices."""
    return [result[k] for k in ("disparity", "uncertainties", "colour", "cloud_counts")] + list(result["cloud"]) + list(result["cloud_index"])


@pytest.mark.parametrize("role", ROLES)
def test_coloured_whole_call_with_each_stream_held(model, timing, role):  # noqa: F811
    if not _CASE or _CASE[0].model is not model or not _CASE[0].current():
        _CASE[:] = [ColourVideoCase(model)]
    case = _CASE[0]
    assert role in case.roles.names(), (role, case.roles.names())
    delay, want, ref = case.reference()
    assert list(want) == ["disparity", "uncertainties", "colour", "cloud", "cloud_counts", "cloud_index"]
    assert tuple(want["colour"].shape) == (7, 60, 250, 4) and len(want["cloud"]) == 7 and sum(want["cloud_counts"].tolist()) > 0
    # the windows' frames differ, so a plane read before it was written, or after the next window's, shows
    assert len({bytes(want["colour"][f].numpy().tobytes()) for f in range(7)}) == 7
    got, ledger = held_run("colour video", role, case.roles, delay, case.run, case.prepare)
    assert ledger.counts == ref.counts, f"{role} held: another path was taken"
    for i, (a, b) in enumerate(zip(flat(got), flat(want))):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{role} held: tensor {i}"
