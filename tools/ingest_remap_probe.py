"""Same-box A/B of rectification at the front door: PPMStereo.forward_batch_test on the raw uint8 frames of an unrectified rig, already on the device,
A: rectified by the caller on the device with RectifyMap.apply_u8 (a chain of torch gathers that writes a second copy of both views), then the
   uint8 path (ppms_video_ingest_u8);
B: with rectify= (ppms_video_ingest_u8_remap: the remap happens where the ingest kernel fetches its bytes).
    python tools/ingest_remap_probe.py [--runs 12] [--yuv] > profiles/rNN_ingest_remap_ab.txt
Two worker processes of this tree stay alive and take turns, one whole call each, so both see the same box, clocks and host load.  Per side: median
/ min / max whole-call ms (device video -> host disparity) and a digest of the results, which must be equal.  Config 2: T = 5, rectified 320x512
from a 360x576 source, iters = 10.  --yuv: the raw frames are NV12 (A converts with to_rgb_u8 first; B is ppms_video_ingest_yuv420_remap).
Nothing gates on this tool."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H0, W0, HS, WS, ITERS = 5, 320, 512, 360, 576, 10


# ------------------------------------------------------------------------------------------------------------------------------ worker
def worker(mode: str, yuv: bool):
    sys.path.insert(0, HERE)
    import torch
    from ppmstereo_amd import weights as Wm
    from ppmstereo_amd.ppmstereo import PPMStereo, RectifyMap, StereoRectifier, YUVFrames, YUVStereoVideo
    dev = torch.device("cuda:0")
    m = PPMStereo.shipped()
    m.load_hot_path_weights(Wm.hot_path_weights())
    m.fnet.load_state_dict(Wm.fnet_weights(), strict=True), m.cnet.load_state_dict(Wm.cnet_weights(), strict=True)
    sd = m.state_dict()
    sd.update(Wm.sst_weights())
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    say = lambda *a: print(*a, flush=True)

    ys, xs = torch.meshgrid(torch.arange(H0, dtype=torch.float32), torch.arange(W0, dtype=torch.float32), indexing="ij")
    maps = []
    for i in range(2):                                          # a resize folded into a mild barrel-like warp, distinct per view
        u, v = (xs - W0 / 2) / (W0 / 2), (ys - H0 / 2) / (H0 / 2)
        k = 1.0 + (0.03 + 0.01 * i) * (u * u + v * v)
        maps.append(RectifyMap.from_float(WS / 2 + u * k * (WS / 2 - 4) + i, HS / 2 + v * k * (HS / 2 - 4), (HS, WS)))
    rect = StereoRectifier(*maps).to(dev)
    raw = Wm.hash_uniform((T, 2, 3, HS, WS), 613, 0.0, 255.0).round().to(torch.uint8).to(dev)
    if yuv:
        planes = lambda s: YUVFrames.nv12(raw[:, s, 0].contiguous(), raw[:, s, 1:, ::2, ::2].permute(0, 2, 3, 1).contiguous())
        raw = YUVStereoVideo(planes(0), planes(1))

    def call():
        if mode == "remap":
            return m.forward_batch_test({"stereo_video": raw}, kernel_size=20, iters=ITERS, rectify=rect)
        left, right = (raw.left.to_rgb_u8(), raw.right.to_rgb_u8()) if yuv else (raw[:, 0], raw[:, 1])
        video = torch.stack(rect.apply_u8(left, right), dim=1)
        return m.forward_batch_test({"stereo_video": video}, kernel_size=20, iters=ITERS)

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
    def __init__(self, label, mode, yuv):
        self.label = label
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode] + (["--yuv"] if yuv else [])
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
    ap.add_argument("--yuv", action="store_true", help="NV12 raw frames instead of planar RGB bytes")
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.yuv)
    A = Side("RectifyMap.apply_u8 on the device, then the uint8 path", "apply", a.yuv)
    B = Side("rectify= (the remap inside the ingest kernel)", "remap", a.yuv)
    try:
        for s in (A, B):
            s.ask()                                             # "ready": the model is built and warm
        ms = {A: [], B: []}
        for _ in range(a.runs):
            for s in (A, B):                                    # alternate: one whole call each
                ms[s].append(float(s.ask("run")[0]))
        sums = {s: s.ask("sum")[0] for s in (A, B)}
        print(f"== T = {T}, {'NV12' if a.yuv else 'RGB'} source {HS}x{WS} -> rectified {H0}x{W0}, iters = {ITERS}: forward_batch_test(device video) -> "
              f"host disparity, {a.runs} alternating calls per side")
        for s in (A, B):
            v = ms[s]
            print(f"{s.label}:")
            print(f"    whole call ms: median {statistics.median(v):.2f}  min {min(v):.2f}  max {max(v):.2f}   [{' '.join(f'{x:.1f}' for x in v)}]")
            print(f"    sha256 of disparity + uncertainties: {sums[s]}")
        ma, mb = statistics.median(ms[A]), statistics.median(ms[B])
        print(f"rectify= median / apply_u8 median = {mb / ma:.4f} ({mb - ma:+.2f} ms); results {'bit-identical' if sums[A] == sums[B] else 'DIFFER'}")
        print("host: cpus", os.cpu_count(), "loadavg", os.getloadavg())
    finally:
        for s in (A, B):
            s.close()


if __name__ == "__main__":
    main()
