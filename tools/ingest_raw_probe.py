"""Same-box A/B of the raw-sensor front door: PPMStereo.forward_batch_test on Bayer-mosaic (or monochrome) frames of 8, 10 or 12 bits, already on
the device,
A: demosaiced by the caller on the device with RawFrames.to_rgb() (torch integer ops), then the door those levels fit: the uint8 door at depth 8
   (3 bytes per pixel and view written and read again), the float door on to_float() at depth 10 / 12 (12 bytes per pixel and view);
B: the RawStereoVideo itself (ppms_video_ingest_raw: demosaic, black level and white balance happen where the ingest kernel fetches its samples, the
   level table of 2^depth entries sits in LDS).
    python tools/ingest_raw_probe.py [--runs 12] [--depth 10] [--pattern rggb] [--align lsb] > profiles/rNN_ingest_raw_ab.txt
Two worker processes of this tree stay alive and take turns, one whole call each, so both see the same box, clocks and host load.  Every step that
uses the GPU -- a worker's start-up, each timed call, each digest -- has its own time limit, and the first step that fails, faults or runs out of
time ends the probe: nothing more is started on the device.  Per side: median / min / max whole-call ms (device video -> host disparity) and a
digest of the results, which must be equal.  Config 2: T = 5, 320x512, iters = 10.  No ratio is promised; nothing gates on this tool."""
import argparse
import hashlib
import os
import select
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H0, W0, ITERS = 5, 320, 512, 10
START_S, CALL_S = 300.0, 60.0                                   # time limits: building + warming a worker; one call or digest


# ------------------------------------------------------------------------------------------------------------------------------ worker
def worker(mode: str, depth: int, pattern: str, align: str):
    sys.path.insert(0, HERE)
    import torch
    from ppmstereo_amd import weights as Wm
    from ppmstereo_amd.ppmstereo import PPMStereo, RawFrames, RawStereoVideo
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
    samples = Wm.hash_uniform((T, 2, H0, W0), 618, 0.0, float(top)).round().to(torch.int32)
    word = (lambda t: t.to(torch.uint8)) if depth == 8 else (lambda t: (t << (16 - depth if align == "msb" else 0)).to(torch.uint16))
    view = lambda s: RawFrames(word(samples[:, s]).contiguous().to(dev), pattern, depth, align, black=top // 16, gains=(1.8, 1.0, 1.5))
    video = RawStereoVideo(view(0), view(1))

    def call():
        if mode == "door":
            return m.forward_batch_test({"stereo_video": video}, kernel_size=20, iters=ITERS)
        frames = (lambda v: v.to_rgb()) if depth == 8 else (lambda v: v.to_float())
        return m.forward_batch_test({"stereo_video": torch.stack([frames(video.left), frames(video.right)], dim=1)}, kernel_size=20, iters=ITERS)

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
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--depth", str(a.depth), "--pattern", a.pattern, "--align", a.align]
        self.p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(self, limit, *cmd):
        """One step of the worker under its own time limit; a worker that ends, or says nothing in time, ends the probe (RuntimeError)."""
        if cmd:
            self.p.stdin.write(" ".join(map(str, cmd)) + "\n")
            self.p.stdin.flush()
        end = time.monotonic() + limit
        while True:
            left = end - time.monotonic()
            if left <= 0 or not select.select([self.p.stdout], [], [], left)[0]:
                raise RuntimeError(f"worker '{self.label}' did not answer {' '.join(map(str, cmd)) or 'ready'!r} within {limit:.0f} s")
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"worker '{self.label}' ended (exit {self.p.wait()})")
            parts = line.split()
            if parts and parts[0] in ("ready", "ms", "sum"):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--depth", type=int, default=10, choices=(8, 10, 12))
    ap.add_argument("--pattern", default="rggb", choices=("rggb", "bggr", "grbg", "gbrg", "mono"))
    ap.add_argument("--align", default="lsb", choices=("msb", "lsb"))
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.depth, a.pattern, a.align)
    sides, failed = [], True
    try:
        # one worker at a time is started and warmed: the second only once the first has answered
        for label, mode in ((f"RawFrames.to_rgb() on the device, then the {'uint8' if a.depth == 8 else 'float'} door", "torch"),
                            ("the RawStereoVideo itself (ppms_video_ingest_raw)", "door")):
            sides.append(Side(label, mode, a))
            sides[-1].ask(START_S)                              # "ready": the model is built and warm
        A, B = sides
        ms = {A: [], B: []}
        for _ in range(a.runs):
            for s in (A, B):                                    # alternate: one whole call each
                ms[s].append(float(s.ask(CALL_S, "run")[0]))
        sums = {s: s.ask(CALL_S, "sum")[0] for s in (A, B)}
        failed = False
        print(f"== T = {T}, {a.depth}-bit {a.pattern} frames ({a.align}) {H0}x{W0}, iters = {ITERS}: forward_batch_test(device video) -> host disparity, "
              f"{a.runs} alternating calls per side")
        for s in (A, B):
            v = ms[s]
            print(f"{s.label}:")
            print(f"    whole call ms: median {statistics.median(v):.2f}  min {min(v):.2f}  max {max(v):.2f}   [{' '.join(f'{x:.1f}' for x in v)}]")
            print(f"    sha256 of disparity + uncertainties: {sums[s]}")
        ma, mb = statistics.median(ms[A]), statistics.median(ms[B])
        print(f"door median / torch-demosaic median = {mb / ma:.4f} ({mb - ma:+.2f} ms); results {'bit-identical' if sums[A] == sums[B] else 'DIFFER'}")
        print("host: cpus", os.cpu_count(), "loadavg", os.getloadavg())
    finally:
        for s in sides:
            s.close(failed)


if __name__ == "__main__":
    main()
