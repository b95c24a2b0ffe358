"""CPU: what becomes of a window's result in forward_batch_test (ppmstereo_amd.output: _PlaneSink, _Float32Sink).  The sinks are host logic: here
they take seeded CPU tensors window by window, into ordinary (unpinned) host buffers, and every key of the dict they return is compared with an
assembly written out plainly.  No device; every comparison is exact."""
import torch

from ppmstereo_amd.output import OutputSpec, _Float32Sink, _PlaneSink, egress_plan
from ppmstereo_amd.video import InputPadder, window_plan

N, CAPACITY = 7, 6
COUNTS = [0, 2, 6, 9, 5, 6, 0]                          # per frame: none, below the capacity, exactly 6, above it (9)
SENTINEL = -7.0


def windows():
    plan = egress_plan(window_plan(N, 4))
    assert sorted({stop - start for start, stop, *_ in plan}) == [3, 4]                    # T = 4 and T = 3
    assert [dst for *_, dst_from, dst_to in plan for dst in range(dst_from, dst_to)] == list(range(N))          # every frame kept once, in order
    assert all(keep_to - keep_from == dst_to - dst_from and dst_from == start + keep_from for start, _, keep_from, keep_to, dst_from, dst_to in plan)
    return plan


def test_plane_sink_fills_its_slices_and_copies_only_the_records_that_exist():
    h0, w0 = 4, 5
    spec = OutputSpec(disparity="u16", uncertainty="u8", points="f32", Q=torch.eye(4), cloud="f32", cloud_index=True, cloud_capacity=CAPACITY)
    assert spec.cloud_components == 3 and list(spec.formats()) == ["disparity", "uncertainties", "points", "cloud", "cloud_counts", "cloud_index"]
    g = torch.Generator().manual_seed(29)
    video = {"disparity": torch.randint(0, 65536, (N, 1, h0, w0), generator=g, dtype=torch.int32).to(torch.uint16),
             "uncertainties": torch.randint(0, 256, (N, 1, h0, w0), generator=g, dtype=torch.int32).to(torch.uint8),
             "points": torch.randn(N, h0, w0, 3, generator=g),
             "cloud": torch.randn(N, CAPACITY, 3, generator=g),               # (rows past a frame's records: whatever the device holds)
             "cloud_counts": torch.tensor(COUNTS, dtype=torch.int32),
             "cloud_index": torch.randint(0, h0 * w0, (N, CAPACITY), generator=g, dtype=torch.int32)}
    sink = _PlaneSink(spec, N, h0, w0, pin_memory=False)
    assert {k: (tuple(v.shape), v.dtype) for k, v in sink.host.items()} == {k: (tuple(v.shape), v.dtype) for k, v in video.items()}
    buffers = {k: sink.host[k] for k in ("cloud", "cloud_index")}
    for buf in buffers.values():
        buf.fill_(SENTINEL)
    for _, _, keep_from, keep_to, dst_from, dst_to in windows():
        planes = {k: v[dst_from:dst_to][None].clone() for k, v in video.items()}            # a window's result: its kept frames, (1, n, ...)
        sink.take(planes, None, keep_from, keep_to, dst_from, dst_to)
    out = sink.result()
    assert list(out) == list(video)
    for key in ("disparity", "uncertainties", "points"):
        assert out[key].dtype == video[key].dtype and torch.equal(out[key], video[key]), key
    assert out["cloud_counts"].dtype == torch.int64 and out["cloud_counts"].tolist() == COUNTS          # the 9 is kept
    for key, buf in buffers.items():
        assert isinstance(out[key], list) and len(out[key]) == N
        for f, count in enumerate(COUNTS):
            k = min(count, CAPACITY)
            assert tuple(out[key][f].shape) == (k, 3)[:video[key].dim() - 1] and torch.equal(out[key][f], video[key][f, :k]), (key, f)
            assert bool((buf[f, k:] == SENTINEL).all()), (key, f, "a record past the frame's count was copied")


def test_float32_sink_keeps_the_unpadded_centre_frames():
    h0, w0 = 6, 10
    padder = InputPadder((h0, w0), divis_by=4)
    left, top, H, W = padder.geometry()
    assert (H, W) == (8, 12) and (left, top) == (1, 1)                                      # it pads for real
    g = torch.Generator().manual_seed(31)
    disp, unc = torch.randn(N, 1, H, W, generator=g), torch.randn(N, 1, H, W, generator=g)   # the padded video's frames, both signs
    sink = _Float32Sink()
    for start, stop, keep_from, keep_to, dst_from, dst_to in windows():
        result = (disp[start:stop][None].clone(), unc[start:stop][None].clone())            # (1, T, 1, H, W) each
        sink.take(result, padder, keep_from, keep_to, dst_from, dst_to)
    out = sink.result()
    assert list(out) == ["disparity", "uncertainties"]
    for key, x in (("disparity", disp), ("uncertainties", unc)):
        want = x[:, :1, top:top + h0, left:left + w0].abs()
        assert tuple(out[key].shape) == (N, 1, h0, w0) and torch.equal(out[key], want), key
