"""Same-box A/B of the video front doors, and of the ingest kernels alone.

    python tools/ingest_probe.py --door u8    [--parent DIR] [--large] [--runs 12]                      > profiles/rNN_ingest_u8_ab.txt
    python tools/ingest_probe.py --door yuv   [--runs 12]                                               > profiles/rNN_ingest_yuv_ab.txt
    python tools/ingest_probe.py --door remap [--yuv] [--runs 12]                                       > profiles/rNN_ingest_remap_ab.txt
    python tools/ingest_probe.py --door deep  [--depth 10] [--chroma 420] [--align msb] [--runs 12]     > profiles/rNN_ingest_deep_ab.txt
    python tools/ingest_probe.py --door raw   [--depth 10] [--pattern rggb] [--align lsb] [--runs 12]   > profiles/rNN_ingest_raw_ab.txt
    python tools/ingest_probe.py --door packed [--layout yuyv | ... | v210 | mipi | pfnc] [--depth 10]  > profiles/rNN_ingest_packed_ab.txt
    python tools/ingest_probe.py --door rgb   [--layout bgr24 | bgra | ... | rgb48 | x2rgb10] [--depth 10] > profiles/rNN_ingest_rgb_ab.txt
    python tools/ingest_probe.py --kernels --parent DIR [--runs 7]                                      > profiles/rNN_ingest_kernels_ab.txt

--door: PPMStereo.forward_batch_test on one video through two ways in.  Side B is the door itself; side A is what a caller did before the door
existed (DOORS below says it per door).  Config 2: T = 5, 320x512, iters = 10; whole-call ms (video -> host disparity) and a digest of the
results, which must be equal.  --parent DIR (a checkout of an earlier commit with its library built): --door u8 runs side A in that tree, every other door runs the door
itself in both trees (A: the parent's host path, B: this tree's); --large
(u8 only) adds one window of 720x1280.  No ratio is promised; nothing gates on these numbers.

--kernels: no whole calls.  A worker in --parent DIR and one in this tree time each of the 8 ppms_video_ingest_* entry points alone through the C ABI,
in every sample format it accepts: N = 5 frames of 320x512 per view (a multiple of 32: the model adds no padding), both destinations, the _remap twins
from a 360x576 source.  Per row: a warm-up, then --runs windows per worker of 300 back-to-back launches between two events, the workers taking
turns window by window.  The yardstick is the parent: its median and the range its own windows span; this tree's median; and whether the digests of
the operands both wrote are equal.

Two worker processes stay alive and take turns, so both see the same box, clocks and host load.  One worker at a time is started and warmed.
Every step that uses the GPU -- a worker's start-up, each timed call or window, each digest -- has its own time limit, and the first step that
fails, faults or runs out of time ends the probe: nothing more is started on the device."""
import argparse
import hashlib
import os
import select
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H0, W0, HS, WS, ITERS = 5, 320, 512, 360, 576, 10
START_S, CALL_S = 300.0, 60.0                                   # time limits: building + warming a worker; one call, window or digest
LAUNCHES = 300                                                  # --kernels: launches per timed window


def words(torch, t, depth, align):
    """Integer samples of `depth` bits as a decoder or driver stores them: bytes, or 16-bit words with the sample at the top or the bottom."""
    return t.to(torch.uint8) if depth == 8 else (t << (16 - depth if align == "msb" else 0)).to(torch.uint16)


def rectifier(torch, P, dev):
    """A resize from HS x WS folded into a mild barrel-like warp, distinct per view."""
    ys, xs = torch.meshgrid(torch.arange(H0, dtype=torch.float32), torch.arange(W0, dtype=torch.float32), indexing="ij")
    maps = []
    for i in range(2):
        u, v = (xs - W0 / 2) / (W0 / 2), (ys - H0 / 2) / (H0 / 2)
        k = 1.0 + (0.03 + 0.01 * i) * (u * u + v * v)
        maps.append(P.RectifyMap.from_float(WS / 2 + u * k * (WS / 2 - 4) + i, HS / 2 + v * k * (HS / 2 - 4), (HS, WS)))
    return P.StereoRectifier(*maps).to(dev)


# ------------------------------------------------------------------------------------------------------------------------------ the doors
# Per door: video(a, torch, P, Wm, dev, h, w) -> (what side B hands to forward_batch_test, its keyword arguments), and
# side_a(a, torch, P, video, kw) -> the same pair for side A, made from B's video inside the timed call (u8: once, before: a float video on the host
# is what that caller starts from).  (P: the ppmstereo module.)
def u8_video(a, torch, P, Wm, dev, h, w):
    return Wm.hash_uniform((T, 2, 3, h, w), 613, 0.0, 255.0).round().contiguous().to(torch.uint8), {}     # on the HOST: the copy is part of the call


def nv12_pair(torch, P, rgb):
    planes = lambda s: P.YUVFrames.nv12(rgb[:, s, 0].contiguous(), rgb[:, s, 1:, ::2, ::2].permute(0, 2, 3, 1).contiguous())
    return P.YUVStereoVideo(planes(0), planes(1))                 # (planes 0, 1, 2 of a view stand for Y, U, V)


def yuv_video(a, torch, P, Wm, dev, h, w):
    return nv12_pair(torch, P, Wm.hash_uniform((T, 2, 3, h, w), 613, 0.0, 255.0).round().to(torch.uint8).to(dev)), {}


def remap_video(a, torch, P, Wm, dev, h, w):
    raw = Wm.hash_uniform((T, 2, 3, HS, WS), 613, 0.0, 255.0).round().to(torch.uint8).to(dev)
    return (nv12_pair(torch, P, raw) if a.yuv else raw), {"rectify": rectifier(torch, P, dev)}


def remap_side_a(a, torch, P, video, kw):
    left, right = (video.left.to_rgb_u8(), video.right.to_rgb_u8()) if a.yuv else (video[:, 0], video[:, 1])
    return torch.stack(kw["rectify"].apply_u8(left, right), dim=1), {}


def deep_video(a, torch, P, Wm, dev, h, w):
    top = (1 << a.depth) - 1
    raw = Wm.hash_uniform((T, 2, 3, h, w), 617, 0.0, float(top)).round().to(torch.int32)
    sy, sx = {"420": (2, 2), "422": (1, 2), "444": (1, 1)}[a.chroma]
    plane = lambda s, c, ry, rx: words(torch, raw[:, s, c, ::ry, ::rx], a.depth, a.align).contiguous().to(dev)
    view = lambda s: P.YUVFrames.planar(plane(s, 0, 1, 1), plane(s, 1, sy, sx), plane(s, 2, sy, sx), depth=a.depth, chroma=a.chroma, align=a.align)
    return P.YUVStereoVideo(view(0), view(1)), {}


def raw_video(a, torch, P, Wm, dev, h, w):
    top = (1 << a.depth) - 1
    samples = Wm.hash_uniform((T, 2, h, w), 618, 0.0, float(top)).round().to(torch.int32)
    view = lambda s: P.RawFrames(words(torch, samples[:, s], a.depth, a.align).contiguous().to(dev), a.pattern, a.depth, a.align, black=top // 16,
                                 gains=(1.8, 1.0, 1.5))
    return P.RawStereoVideo(view(0), view(1)), {}


YUV_LAYOUTS = {"yuyv": 8, "uyvy": 8, "yvyu": 8, "vyuy": 8, "y210": 10, "y212": 12, "v210": 10}            # layout: depth
RAW_PACKINGS = ("mipi", "pfnc")                                  # (--depth 10 | 12, --pattern)


def packed_video(a, torch, P, Wm, dev, h, w):
    """The frames of --door deep (4:2:2) or --door raw, packed on the host with the classes' own pack() and moved to the device as packed bytes."""
    if a.layout in RAW_PACKINGS:
        depth = a.depth if a.depth in (10, 12) else 10
        top = (1 << depth) - 1
        samples = Wm.hash_uniform((T, 2, h, w), 618, 0.0, float(top)).round().to(torch.int32)
        view = lambda s: P.PackedRawFrames.pack(P.RawFrames(samples[:, s].to(torch.uint16).contiguous(), a.pattern, depth, "lsb", black=top // 16,
                                                            gains=(1.8, 1.0, 1.5)), a.layout).to(dev)
        return P.PackedRawStereoVideo(view(0), view(1)), {}
    depth = YUV_LAYOUTS[a.layout]
    raw = Wm.hash_uniform((T, 2, 3, h, w), 617, 0.0, float((1 << depth) - 1)).round().to(torch.int32)
    plane = lambda s, c, rx: words(torch, raw[:, s, c, :, ::rx], depth, "lsb").contiguous()
    view = lambda s: P.PackedYUVFrames.pack(P.YUVFrames.planar(plane(s, 0, 1), plane(s, 1, 2), plane(s, 2, 2), depth=depth, chroma="422"), a.layout).to(dev)
    return P.PackedYUVStereoVideo(view(0), view(1)), {}


def packed_side_a(a, torch, P, video, kw):                      # what a caller did before the door: unpack in torch, then the unpacked door
    video_of = P.PackedRawStereoVideo if a.layout in RAW_PACKINGS else P.PackedYUVStereoVideo
    assert isinstance(video, video_of)
    return (P.RawStereoVideo if a.layout in RAW_PACKINGS else P.YUVStereoVideo)(video.left.unpack(), video.right.unpack()), {}


RGB_LAYOUTS = {"rgb24": 8, "bgr24": 8, "rgba": 8, "bgra": 8, "argb": 8, "abgr": 8, "rgb48": 0, "bgr48": 0, "rgba64": 0, "bgra64": 0,
               "x2rgb10": 10, "x2bgr10": 10}                    # layout: depth (0: --depth 10 | 12, in 16-bit words, --align)


def rgb_depth(a):
    return RGB_LAYOUTS[a.layout] or (a.depth if a.depth in (10, 12) else 10)


def rgb_bytes(a):
    """Bytes per pixel and view that cross into the ingest launch, by construction: side B's own pixels, and what side A's planar video (uint8,
    or float32 for the deep layouts) is written and read with on top of them."""
    step = 3 if a.layout in ("rgb24", "bgr24", "rgb48", "bgr48") else 4
    own = 4 if a.layout.startswith("x2") else step * (1 if rgb_depth(a) == 8 else 2)
    return own, 3 if rgb_depth(a) == 8 else 12


def rgb_video(a, torch, P, Wm, dev, h, w):
    """Interleaved frames, packed on the host with the class's own pack() and moved to the device as they are."""
    depth = rgb_depth(a)
    levels = Wm.hash_uniform((T, 2, 3, h, w), 619, 0.0, float((1 << depth) - 1)).round().to(torch.uint8 if depth == 8 else torch.int16)
    view = lambda s: P.PackedRGBFrames.pack(levels[:, s].contiguous(), a.layout, depth, a.align).to(dev)
    return P.PackedRGBStereoVideo(view(0), view(1)), {}


def rgb_side_a(a, torch, P, video, kw):                         # what a caller did before the door: the transposing copy in front of forward
    assert isinstance(video, P.PackedRGBStereoVideo)
    if video.depth > 8:
        return torch.stack([video.left.to_float(), video.right.to_float()], dim=1), {}
    hwc = lambda v: v.data.unflatten(2, (v.width, v.step))       # (N, H, W, C): the caller's own tensor
    return torch.stack([hwc(v).permute(0, 3, 1, 2)[:, list(v.offset)].contiguous() for v in (video.left, video.right)], dim=1), {}


def levels_side_a(a, torch, P, video, kw):                      # the uint8 door where the levels are bytes, the float door on to_float() otherwise
    frames = (lambda v: v.to_rgb()) if a.depth == 8 else (lambda v: v.to_float())
    return torch.stack([frames(video.left), frames(video.right)], dim=1), {}


DOORS = {  # door: (video, side_a, what side A is, what side B is[, side A's video is made once])
    "u8": (u8_video, lambda a, torch, P, video, kw: (video.float(), {}), "float32 video", "uint8 video (ppms_video_ingest_u8)", True),
    "yuv": (yuv_video, lambda a, torch, P, video, kw: (torch.stack([video.left.to_rgb_u8(), video.right.to_rgb_u8()], dim=1), {}),
            "YUVFrames.to_rgb_u8() on the device, then the uint8 door", "the NV12 YUVStereoVideo itself (ppms_video_ingest_yuv420)"),
    "remap": (remap_video, remap_side_a, "RectifyMap.apply_u8 on the device, then the uint8 door", "rectify= (the remap inside the ingest kernel)"),
    "deep": (deep_video, lambda a, torch, P, video, kw: (torch.stack([video.left.to_float(), video.right.to_float()], dim=1), {}),
             "YUVFrames.to_float() on the device, then the float door", "the YUVStereoVideo itself (ppms_video_ingest_yuv)"),
    "raw": (raw_video, levels_side_a, "RawFrames.to_rgb() / to_float() on the device, then the uint8 / float door",
            "the RawStereoVideo itself (ppms_video_ingest_raw)"),
    "packed": (packed_video, packed_side_a, "unpack() in torch on the device, then the unpacked door (ppms_video_ingest_yuv / ppms_video_ingest_raw)",
               "the packed stereo video itself (ppms_video_ingest_yuv_packed / ppms_video_ingest_raw_packed)"),
    "rgb": (rgb_video, rgb_side_a, "frames.permute(0, 3, 1, 2)[:, order].contiguous() on the device, then the uint8 door (deep layouts: to_float(), the float door)",
            "the interleaved frames themselves (ppms_video_ingest_rgb_packed)"),
}


# ------------------------------------------------------------------------------------------------------------------------------ workers
def serve(handlers):
    """The worker loop: one command per line of stdin, one answer line each."""
    for line in sys.stdin:
        cmd = line.split()
        if cmd and cmd[0] == "quit":
            break
        if cmd:
            print(cmd[0], *handlers[cmd[0]](*cmd[1:]), flush=True)


def door_worker(a, tree):
    sys.path.insert(0, tree)
    import torch
    from ppmstereo_amd import _lib as L
    from ppmstereo_amd import ppmstereo as P
    from ppmstereo_amd import weights as Wm
    assert os.path.dirname(os.path.dirname(os.path.abspath(L.__file__))) == os.path.abspath(tree), (L.__file__, tree)
    dev = torch.device("cuda:0")
    m = P.PPMStereo.shipped()
    m.load_hot_path_weights(Wm.hot_path_weights())
    m.fnet.load_state_dict(Wm.fnet_weights(), strict=True), m.cnet.load_state_dict(Wm.cnet_weights(), strict=True)
    sd = m.state_dict()
    sd.update(Wm.sst_weights())
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    make_video, side_a, once = DOORS[a.door][0], DOORS[a.door][1], len(DOORS[a.door]) > 4
    state = {}

    def call():
        video, kw = state["video"]
        if a.worker == "A" and not once:
            video, kw = side_a(a, torch, P, video, kw)
        return m.forward_batch_test({"stereo_video": video}, kernel_size=20, iters=ITERS, **kw)

    def setup(h, w):
        state["video"] = make_video(a, torch, P, Wm, dev, int(h), int(w))
        if a.worker == "A" and once:
            state["video"] = side_a(a, torch, P, *state["video"])
        for _ in range(3):
            state["out"] = call()
        torch.cuda.synchronize()
        return ()

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        state["out"] = call()
        return (f"{1e3 * (time.perf_counter() - t0):.3f}",)

    def digest():
        out = state["out"]
        return (hashlib.sha256(out["disparity"].contiguous().numpy().tobytes() + out["uncertainties"].contiguous().numpy().tobytes()).hexdigest()[:16],)

    def count():
        """One call with Python-level hooks that the timed calls never see: host->device bytes, and the device work enqueued on the caller's
        stream between the host->device copy and fnet's first convolution (torch ops that launch + library launches)."""
        from torch.utils._python_dispatch import TorchDispatchMode
        from ppmstereo_amd import convplan
        events, h2d = [], [0]
        stream = lambda: torch.cuda.current_stream(dev).cuda_stream

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                name = func._schema.name
                view = any(r.alias_info is not None and not r.alias_info.is_write for r in func._schema.returns)
                src = args[0] if args and torch.is_tensor(args[0]) else None
                if torch.is_tensor(out) and out.is_cuda and src is not None and not src.is_cuda and name in ("aten::_to_copy", "aten::copy_"):
                    h2d[0] += src.numel() * src.element_size()
                    events.append((stream(), "h2d", name))
                elif not view and torch.is_tensor(out) and out.is_cuda and not name.startswith(("aten::empty", "aten::new_empty")):
                    events.append((stream(), "op", name))
                return out

        saved = []
        for cls in {c for c in vars(convplan).values() if isinstance(c, type) and "__call__" in vars(c)}:
            orig = cls.__call__
            saved.append((cls, orig))
            cls.__call__ = (lambda orig: lambda self, *a, **k: (events.append((stream(), "conv", type(self).__name__)), orig(self, *a, **k))[1])(orig)
        lib = L.load()
        for name in ("ppms_img_s2d", "ppms_video_ingest_u8"):
            if hasattr(lib, name):
                fn = getattr(lib, name)
                setattr(lib, name, (lambda fn, name: lambda *a: (events.append((stream(), "lib", name)), fn(*a))[1])(fn, name))
        caller = stream()
        with Mode():
            call()
        for cls, orig in saved:
            cls.__call__ = orig
        mine = [e for e in events if e[0] == caller]
        first_h2d = next((i for i, e in enumerate(mine) if e[1] == "h2d"), -1)
        first_conv = next(i for i, e in enumerate(mine) if e[1] == "conv")
        between = [e[2] for e in mine[first_h2d + 1:first_conv]]
        side = [e for e in events if e[0] != caller]
        return h2d[0], len(between), next((i for i, e in enumerate(side) if e[1] == "conv"), len(side)), ",".join(n.replace("aten::", "") for n in between)

    print("ready", flush=True)
    serve({"setup": setup, "run": run, "sum": digest, "count": count})


# the rows of --kernels: (entry point, sample_bytes, depth, lsb), each also as the _remap twin
SAMPLES = [(1, 8, 0), (2, 10, 0), (2, 10, 6), (2, 12, 0), (2, 12, 4)]
ROWS = [(e + tw, *s) for e, fmts in (("u8", SAMPLES[:1]), ("yuv420", SAMPLES[:1]), ("yuv", SAMPLES), ("raw", SAMPLES)) for tw in ("", "_remap") for s in fmts]


def kernels_worker(a, tree):
    sys.path.insert(0, tree)
    import ctypes
    import torch
    from ppmstereo_amd import _lib as L
    from ppmstereo_amd import ppmstereo as P
    assert os.path.dirname(os.path.dirname(os.path.abspath(L.__file__))) == os.path.abspath(tree), (L.__file__, tree)
    lib, dev, ref = L.load(), torch.device("cuda:0"), ctypes.byref
    rect = rectifier(torch, P, dev)
    plane = lambda shape, seed: torch.randint(0, 1 << 16, shape, dtype=torch.int32, generator=torch.Generator().manual_seed(seed))
    dst = [torch.zeros((n * (H0 // k) * (W0 // k), c), dtype=torch.int16, device=dev) for n, k, c in ((2 * T, 2, 32), (2 * T, 2, 32), (T, 4, 64), (T, 4, 64))]
    sp = [L.SP(dst[0].data_ptr(), dst[1].data_ptr(), 32, 32), L.SP(dst[2].data_ptr(), dst[3].data_ptr(), 64, 64)]
    calls = {}

    def prep(i):
        """Builds row i's call on frames of random samples, warms it up and answers with the digest of both destinations' planes."""
        name, sb, depth, lsb = ROWS[int(i)]
        entry, remap = name.replace("_remap", ""), name.endswith("_remap")
        h, w = (HS, WS) if remap else (H0, W0)
        dt = torch.uint8 if sb == 1 else torch.uint16
        hold = [(plane(s, 7 + k) & ((1 << (8 * sb)) - 1)).to(dt).to(dev) for k, s in
                enumerate(((T, 3, h, w),) * 2 if entry == "u8" else ((T, h, w),) * 2 if entry == "raw" else ((T, h, w), (T, h // 2, w // 2), (T, h // 2, w // 2)) * 2)]
        if entry == "u8":
            head = [hold[0].data_ptr(), hold[1].data_ptr(), 3 * h * w]
        elif entry == "raw":
            fmt = L.RawFormat(sb, depth, lsb, 0, ((1 << depth) - 1) // 16, (1843, 1024, 1536), 10, (0, 0, 0))
            head = [L.RawView(t.data_ptr(), h * w * sb, w * sb, 0) for t in hold] + [fmt]
        else:
            view = lambda y, u, v: L.YUVView(y.data_ptr(), u.data_ptr(), v.data_ptr(), h * w * sb, (h // 2) * (w // 2) * sb, w * sb, (w // 2) * sb, sb, 0)
            head = [view(*hold[:3]), view(*hold[3:]), P.yuv_matrix(depth=depth)] + ([L.YUVFormat(sb, depth, lsb, 1, 1, (0, 0, 0))] if entry == "yuv" else [])
        maps = [rect.left.view_struct(depth), rect.right.view_struct(depth)] if remap else []
        table = (2 * (torch.arange(1 << depth, dtype=torch.float32, device=dev) / float((1 << depth) - 1)) - 1.0).contiguous()
        args = [x if isinstance(x, int) else ref(x) for x in head + maps] + [T, H0, W0, 0, 0, H0, W0, table.data_ptr(), sp[0], sp[1]]
        fn = getattr(lib, "ppms_video_ingest_" + name)
        calls[int(i)] = (lambda: L.check(fn(*args, L.stream_ptr())), hold, head, maps, table)
        for t in dst:
            t.zero_()
        for _ in range(20):
            calls[int(i)][0]()
        torch.cuda.synchronize()
        return (hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in dst)).hexdigest()[:16],)

    def window(i):
        call = calls[int(i)][0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(10):
            call()
        e0.record()
        for _ in range(LAUNCHES):
            call()
        e1.record()
        e1.synchronize()
        return (f"{1e3 * e0.elapsed_time(e1) / LAUNCHES:.3f}",)

    print("ready", flush=True)
    serve({"prep": prep, "win": window})


# ------------------------------------------------------------------------------------------------------------------------------ driver
class Side:
    def __init__(self, label, a, side, tree):
        self.label = label
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", side, "--tree", tree, "--depth", str(a.depth), "--chroma", a.chroma,
               "--pattern", a.pattern, "--layout", a.layout] + (["--door", a.door] if a.door else ["--kernels"]) + (["--align", a.align] if a.align else []) + (["--yuv"] if a.yuv else [])
        self.p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(self, limit, *cmd):
        """One step of the worker under its own time limit; a worker that ends, or says nothing in time, ends the probe (RuntimeError)."""
        if cmd:
            self.p.stdin.write(" ".join(map(str, cmd)) + "\n")
            self.p.stdin.flush()
        want = cmd[0] if cmd else "ready"
        end = time.monotonic() + limit
        while True:
            left = end - time.monotonic()
            if left <= 0 or not select.select([self.p.stdout], [], [], left)[0]:
                raise RuntimeError(f"worker '{self.label}' did not answer {' '.join(map(str, cmd)) or 'ready'!r} within {limit:.0f} s")
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"worker '{self.label}' ended (exit {self.p.wait()})")
            parts = line.split()
            if parts and parts[0] == want:
                return parts[1:]

    def close(self, failed: bool):
        try:
            if failed:
                self.p.kill()                                    # (a worker that faulted or hangs is not asked for anything more)
            else:
                self.p.stdin.write("quit\n")
                self.p.stdin.close()
        except OSError:
            pass
        try:
            self.p.wait(timeout=60)
        except subprocess.TimeoutExpired:
            self.p.kill()
            self.p.wait()


def door_report(a, A, B):
    for h, w, runs in [(H0, W0, a.runs)] + ([(720, 1280, max(3, a.runs // 3))] if a.large else []):
        for s in (A, B):
            s.ask(START_S, "setup", h, w)
        ms = {A: [], B: []}
        for _ in range(runs):
            for s in (A, B):                                    # alternate: one whole call each
                ms[s].append(float(s.ask(CALL_S, "run")[0]))
        sums = {s: s.ask(CALL_S, "sum")[0] for s in (A, B)}
        fmt = {"u8": "", "yuv": "NV12 ", "remap": f"{'NV12' if a.yuv else 'RGB'} source {HS}x{WS} -> rectified ",
               "deep": f"{a.depth}-bit {a.chroma} planar frames ({a.align}) ", "raw": f"{a.depth}-bit {a.pattern} frames ({a.align}) ",
               "packed": f"{a.layout} frames " + (f"({a.depth if a.depth in (10, 12) else 10}-bit {a.pattern}) " if a.layout in RAW_PACKINGS else ""),
               "rgb": f"{a.layout} frames " + (f"({rgb_depth(a)}-bit, {a.align}) " if a.layout in RGB_LAYOUTS and not RGB_LAYOUTS[a.layout] else "")}[a.door]
        print(f"== --door {a.door}: T = {T}, {fmt}{h}x{w}, iters = {ITERS}: forward_batch_test(video) -> host disparity, {runs} alternating calls per side")
        if a.door == "rgb":
            own, planar = rgb_bytes(a)
            print(f"by construction, not measured: per pixel and view the ingest launch of side B reads the frames' own {own} bytes; side A reads them too, "
                  f"writes {planar} bytes of planar video and its ingest reads those {planar} again")
        for s in (A, B):
            v = ms[s]
            print(f"{s.label}:")
            print(f"    whole call ms: median {statistics.median(v):.2f}  min {min(v):.2f}  max {max(v):.2f}   [{' '.join(f'{x:.1f}' for x in v)}]")
            if a.door == "u8":
                h2d, n, side_n, names = (s.ask(CALL_S, "count") + [""])[:4]
                print(f"    host->device bytes per window: {int(h2d)}")
                print(f"    launches on the caller's stream between the copy and fnet's first convolution: {n}  ({names})")
                print(f"    launches on the side stream before cnet's first convolution: {side_n}")
            print(f"    sha256 of disparity + uncertainties: {sums[s]}")
        ma, mb = statistics.median(ms[A]), statistics.median(ms[B])
        print(f"B median / A median = {mb / ma:.4f} ({mb - ma:+.2f} ms); results {'bit-identical' if sums[A] == sums[B] else 'DIFFER'}")
        print()


def kernels_report(a, A, B):
    print(f"== --kernels: N = {T} frames of {H0}x{W0} per view, both destinations; _remap from {HS}x{WS}; us per launch over windows of {LAUNCHES} launches, "
          f"{a.runs} windows per side, alternating")
    print(f"{'entry':<14} {'bytes':>5} {'depth':>5} {'lsb':>3} | {'parent median':>13} {'min':>8} {'max':>8} | {'this median':>11} {'inside':>6} | digests")
    outside = []
    for i, (name, sb, depth, lsb) in enumerate(ROWS):
        sums = [s.ask(CALL_S, "prep", i)[0] for s in (A, B)]
        us = {A: [], B: []}
        for _ in range(a.runs):
            for s in (A, B):                                    # alternate: one window each
                us[s].append(float(s.ask(CALL_S, "win", i)[0]))
        mb, inside = statistics.median(us[B]), min(us[A]) <= statistics.median(us[B]) <= max(us[A])
        if not inside or sums[0] != sums[1]:
            outside.append(name)
        print(f"{name:<14} {sb:>5} {depth:>5} {lsb:>3} | {statistics.median(us[A]):>13.3f} {min(us[A]):>8.3f} {max(us[A]):>8.3f} | {mb:>11.3f} "
              f"{'yes' if inside else 'NO':>6} | {'equal' if sums[0] == sums[1] else 'DIFFER'} {sums[1]}")
    print(f"rows outside the parent's own range, or with other bits: {', '.join(outside) if outside else 'none'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--door", choices=sorted(DOORS))
    ap.add_argument("--kernels", action="store_true", help="time the 8 entry points alone, --parent DIR against this tree")
    ap.add_argument("--parent", default=None, help="tree of an earlier commit with its libppms.so built (--door u8: side A runs there; other doors: the door itself; --kernels: the yardstick)")
    ap.add_argument("--runs", type=int, default=None, help="alternating calls per side (12), or with --kernels windows per side (7)")
    ap.add_argument("--large", action="store_true", help="--door u8: also one T = 5 window of 720x1280")
    ap.add_argument("--yuv", action="store_true", help="--door remap: NV12 raw frames instead of planar RGB bytes")
    ap.add_argument("--depth", type=int, default=10, choices=(8, 10, 12), help="--door deep / raw")
    ap.add_argument("--chroma", default="420", choices=("420", "422", "444"), help="--door deep")
    ap.add_argument("--align", default=None, choices=("msb", "lsb"), help="--door deep (default msb) / raw (default lsb)")
    ap.add_argument("--pattern", default="rggb", choices=("rggb", "bggr", "grbg", "gbrg", "mono"), help="--door raw")
    ap.add_argument("--layout", default=None, choices=sorted(YUV_LAYOUTS) + list(RAW_PACKINGS) + sorted(RGB_LAYOUTS),
                    help="--door packed (default yuyv; mipi / pfnc: with --depth 10 | 12, --pattern) / rgb (default bgr24; rgb48 ...: with --depth 10 | 12, --align)")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=HERE)
    a = ap.parse_args()
    if bool(a.door) == a.kernels:
        ap.error("one of --door X and --kernels")
    if a.kernels and not a.parent and not a.worker:
        ap.error("--kernels compares against --parent DIR")
    if a.door == "deep" and (a.depth, a.chroma) == (8, "420"):
        ap.error("8-bit 4:2:0 is --door yuv (ppms_video_ingest_yuv420); choose another --depth or --chroma")
    a.align = a.align or ("msb" if a.door in ("deep", "rgb") else "lsb")
    a.layout = a.layout or ("bgr24" if a.door == "rgb" else "yuyv")
    if not a.worker and (a.door == "rgb") != (a.layout in RGB_LAYOUTS) and a.door in ("rgb", "packed"):
        ap.error(f"--layout {a.layout} does not go with --door {a.door}")
    a.runs = a.runs or (7 if a.kernels else 12)
    if a.worker:
        return (kernels_worker if a.kernels else door_worker)(a, os.path.abspath(a.tree))
    ptree = os.path.abspath(a.parent) if a.parent else HERE
    if a.kernels:
        labels = [("the parent's tree", ptree), ("this tree", HERE)]
    else:
        labels = [(DOORS[a.door][2 if a.door == "u8" or not a.parent else 3] + (", the parent's tree" if a.parent else ""), ptree), (DOORS[a.door][3], HERE)]
    sides, failed = [], True
    try:
        for (label, tree), side in zip(labels, "AB" if a.kernels or a.door == "u8" or not a.parent else "BB"):           # one worker at a time is started and warmed: the second only once the first has answered
            sides.append(Side(label, a, side, tree))
            sides[-1].ask(START_S)                              # "ready"
        (kernels_report if a.kernels else door_report)(a, *sides)
        failed = False
        print("host: cpus", os.cpu_count(), "loadavg", os.getloadavg())
    finally:
        for s in sides:
            s.close(failed)


if __name__ == "__main__":
    main()
