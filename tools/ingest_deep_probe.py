"""Same-box A/B of the deep / non-4:2:0 front door: PPMStereo.forward_batch_test on decoded 10- or 12-bit (or 8-bit 4:2:2 / 4:4:4) YUV frames,
already on the device,
A: converted by the caller on the device with YUVFrames.to_float() (torch integer ops that write a float32 video of 12 bytes per pixel and view),
   then the float path (pad, normalise, the two ppms_img_s2d launches);
B: the YUVStereoVideo itself (ppms_video_ingest_yuv: the conversion happens where the ingest kernel fetches its samples, the level table of
   2^depth entries sits in LDS).
    python tools/ingest_deep_probe.py [--runs 12] [--depth 10] [--chroma 420] [--align msb] > profiles/rNN_ingest_deep_ab.txt
Two worker processes of this tree stay alive and take turns, one whole call each, so both see the same box, clocks and host load.  Per side: median
/ min / max whole-call ms (device video -> host disparity) and a digest of the results, which must be equal.  Config 2: T = 5, 320x512, iters = 10.
--depth 8 needs --chroma 422 or 444 (8-bit 4:2:0 is the ppms_video_ingest_yuv420 door).  Nothing gates on this tool."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H0, W0, ITERS = 5, 320, 512, 10


# ------------------------------------------------------------------------------------------------------------------------------ worker
def worker(mode: str, depth: int, chroma: str, align: str):
    sys.path.insert(0, HERE)
    import torch
    from ppmstereo_amd import weights as Wm
    from ppmstereo_amd.ppmstereo import PPMStereo, YUVFrames, YUVStereoVideo
    dev = torch.device("cuda:0")
    m = PPMStereo.shipped()
    m.load_hot_path_weights(Wm.hot_path_weights())
    m.fnet.load_state_dict(Wm.fnet_weights(), strict=True), m.cnet.load_state_dict(Wm.cnet_weights(), strict=True)
    sd = m.state_dict()
    sd.update(Wm.sst_weights())
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    say = lambda *a: print(*a, flush=True)

    top = (1 << depth) - 1
    raw = Wm.hash_uniform((T, 2, 3, H0, W0), 617, 0.0, float(top)).round().to(torch.int32)        # planes 0, 1, 2 of a view stand for Y, U, V
    sy, sx = {"420": (2, 2), "422": (1, 2), "444": (1, 1)}[chroma]
    word = (lambda t: t.to(torch.uint8)) if depth == 8 else (lambda t: (t << (16 - depth if align == "msb" else 0)).to(torch.uint16))
    plane = lambda s, c, ry, rx: word(raw[:, s, c, ::ry, ::rx]).contiguous().to(dev)
    view = lambda s: YUVFrames.planar(plane(s, 0, 1, 1), plane(s, 1, sy, sx), plane(s, 2, sy, sx), depth=depth, chroma=chroma, align=align)
    video = YUVStereoVideo(view(0), view(1))

    def call():
        if mode == "door":
            return m.forward_batch_test({"stereo_video": video}, kernel_size=20, iters=ITERS)
        fl = torch.stack([video.left.to_float(), video.right.to_float()], dim=1)
        return m.forward_batch_test({"stereo_video": fl}, kernel_size=20, iters=ITERS)

    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    say("ready")
    for line in sys.stdin:
        cmd = line.split()
        if not cmd:
            continue
        if cmd[0] == "run":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call()
            say("ms", f"{1e3 * (time.perf_counter() - t0):.3f}")
        elif cmd[0] == "sum":
            d = out["disparity"].contiguous().numpy().tobytes() + out["uncertainties"].contiguous().numpy().tobytes()
            say("sum", hashlib.sha256(d).hexdigest()[:16])
        elif cmd[0] == "quit":
            break


# ------------------------------------------------------------------------------------------------------------------------------ driver
class Side:
    def __init__(self, label, mode, a):
        self.label = label
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--depth", str(a.depth), "--chroma", a.chroma, "--align", a.align]
        self.p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(self, *cmd):
        if cmd:
            self.p.stdin.write(" ".join(map(str, cmd)) + "\n")
            self.p.stdin.flush()
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"worker '{self.label}' ended (exit {self.p.wait()})")
            parts = line.split()
            if parts and parts[0] in ("ready", "ms", "sum"):
                return parts[1:]

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.close()
        except OSError:
            pass
        self.p.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--depth", type=int, default=10, choices=(8, 10, 12))
    ap.add_argument("--chroma", default="420", choices=("420", "422", "444"))
    ap.add_argument("--align", default="msb", choices=("msb", "lsb"))
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if (a.depth, a.chroma) == (8, "420"):
        ap.error("8-bit 4:2:0 is the ppms_video_ingest_yuv420 door; choose another --depth or --chroma")
    if a.worker:
        return worker(a.worker, a.depth, a.chroma, a.align)
    A = Side("YUVFrames.to_float() on the device, then the float path", "float", a)
    B = Side("the YUVStereoVideo itself (ppms_video_ingest_yuv)", "door", a)
    try:
        for s in (A, B):
            s.ask()                                             # "ready": the model is built and warm
        ms = {A: [], B: []}
        for _ in range(a.runs):
            for s in (A, B):                                    # alternate: one whole call each
                ms[s].append(float(s.ask("run")[0]))
        sums = {s: s.ask("sum")[0] for s in (A, B)}
        print(f"== T = {T}, {a.depth}-bit {a.chroma} planar frames ({a.align}) {H0}x{W0}, iters = {ITERS}: forward_batch_test(device video) -> host disparity, "
              f"{a.runs} alternating calls per side")
        for s in (A, B):
            v = ms[s]
            print(f"{s.label}:")
            print(f"    whole call ms: median {statistics.median(v):.2f}  min {min(v):.2f}  max {max(v):.2f}   [{' '.join(f'{x:.1f}' for x in v)}]")
            print(f"    sha256 of disparity + uncertainties: {sums[s]}")
        ma, mb = statistics.median(ms[A]), statistics.median(ms[B])
        print(f"door median / to_float median = {mb / ma:.4f} ({mb - ma:+.2f} ms); results {'bit-identical' if sums[A] == sums[B] else 'DIFFER'}")
        print("host: cpus", os.cpu_count(), "loadavg", os.getloadavg())
    finally:
        for s in (A, B):
            s.close()


if __name__ == "__main__":
    main()
