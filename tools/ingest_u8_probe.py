"""Same-box A/B of the front door: PPMStereo.forward_batch_test on a float32 host video (tree A, --parent DIR: a checkout of the parent commit
with its library built; default: this tree, whose float path is the parent's) against this tree's on the uint8 image of the same video.
    python tools/ingest_u8_probe.py --parent DIR [--runs 12] [--large] > profiles/rNN_ingest_u8_ab.txt
Two worker processes (one per tree) stay alive and take turns, one whole call each, so both see the same box, clocks and host load.  Per side:
median / min / max whole-call ms (host video -> host disparity), host->device bytes per window, and the device work enqueued on the caller's
stream between the host->device copy and fnet's first convolution (torch ops that launch + library launches; counted in one extra call after
the timed ones, with Python-level hooks that the timed calls never see).  Config 2: T = 5, 320x512, iters = 10; --large adds one T = 5 window
of 720x1280."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------------ worker
def worker(tree: str, dtype: str):
    sys.path.insert(0, tree)
    import torch
    from ppmstereo_amd import _lib as L
    from ppmstereo_amd import convplan
    from ppmstereo_amd import weights as Wm
    from ppmstereo_amd.ppmstereo import PPMStereo
    assert os.path.dirname(os.path.dirname(os.path.abspath(L.__file__))) == os.path.abspath(tree), (L.__file__, tree)
    dev = torch.device("cuda:0")
    m = PPMStereo.shipped()
    m.load_hot_path_weights(Wm.hot_path_weights())
    m.fnet.load_state_dict(Wm.fnet_weights(), strict=True), m.cnet.load_state_dict(Wm.cnet_weights(), strict=True)
    sd = m.state_dict()
    sd.update(Wm.sst_weights())
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    say = lambda *a: print(*a, flush=True)
    state = {}

    def setup(T, H, W, iters):
        video = Wm.hash_uniform((T, 2, 3, H, W), 613, 0.0, 255.0).round().contiguous()
        state["video"] = video.to(torch.uint8) if dtype == "u8" else video
        state["call"] = lambda: m.forward_batch_test({"stereo_video": state["video"]}, kernel_size=20, iters=iters)
        for _ in range(3):
            state["call"]()
        torch.cuda.synchronize()

    def count():
        """One call with hooks: every torch op that is neither a view nor an allocation, and every library launch, with the stream it went to."""
        from torch.utils._python_dispatch import TorchDispatchMode
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
            state["call"]()
        for cls, orig in saved:
            cls.__call__ = orig
        mine = [e for e in events if e[0] == caller]
        first_h2d = next((i for i, e in enumerate(mine) if e[1] == "h2d"), -1)
        first_conv = next(i for i, e in enumerate(mine) if e[1] == "conv")
        between = [e[2] for e in mine[first_h2d + 1:first_conv]]
        side = [e for e in events if e[0] != caller]
        side_conv = next((i for i, e in enumerate(side) if e[1] == "conv"), len(side))
        say("count", h2d[0], len(between), side_conv, ",".join(n.replace("aten::", "") for n in between))

    for line in sys.stdin:
        cmd = line.split()
        if not cmd:
            continue
        if cmd[0] == "setup":
            setup(*map(int, cmd[1:5]))
            say("ready", state["video"].numel() * state["video"].element_size())
        elif cmd[0] == "run":
            t0 = time.perf_counter()
            out = state["call"]()
            ms = 1e3 * (time.perf_counter() - t0)
            state["out"] = out
            say("ms", f"{ms:.3f}")
        elif cmd[0] == "sum":
            d = state["out"]["disparity"].contiguous().numpy().tobytes() + state["out"]["uncertainties"].contiguous().numpy().tobytes()
            say("sum", hashlib.sha256(d).hexdigest()[:16])
        elif cmd[0] == "count":
            count()
        elif cmd[0] == "quit":
            break


# ------------------------------------------------------------------------------------------------------------------------------ driver
class Side:
    def __init__(self, label, tree, dtype):
        self.label = label
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", dtype, "--tree", tree], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(self, *cmd):
        self.p.stdin.write(" ".join(map(str, cmd)) + "\n")
        self.p.stdin.flush()
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"worker '{self.label}' ended (exit {self.p.wait()})")
            parts = line.split()
            if parts and parts[0] in ("ready", "ms", "sum", "count"):
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
    ap.add_argument("--parent", default=None, help="tree of the parent commit with its libppms.so built (default: this tree's float path)")
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--large", action="store_true", help="also one T = 5 window of 720x1280")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=HERE)
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.tree), a.worker)
    ptree = os.path.abspath(a.parent) if a.parent else HERE
    A = Side("float32 video, " + ("parent commit's tree" if a.parent else "this tree (float path as in the parent)"), ptree, "f32")
    B = Side("uint8 video, this tree", HERE, "u8")
    try:
        for T, H, W, iters, runs in [(5, 320, 512, 10, a.runs)] + ([(5, 720, 1280, 10, max(3, a.runs // 3))] if a.large else []):
            bytes_ = {s: int(s.ask("setup", T, H, W, iters)[0]) for s in (A, B)}
            ms = {A: [], B: []}
            for _ in range(runs):
                for s in (A, B):                                # alternate: one whole call each
                    ms[s].append(float(s.ask("run")[0]))
            sums = {s: s.ask("sum")[0] for s in (A, B)}
            print(f"== T = {T}, {H}x{W}, iters = {iters}: forward_batch_test(host video) -> host disparity, {runs} alternating calls per side")
            for s in (A, B):
                v = ms[s]
                h2d, n, side_n, names = (s.ask("count") + [""])[:4]
                print(f"{s.label}:")
                print(f"    whole call ms: median {statistics.median(v):.2f}  min {min(v):.2f}  max {max(v):.2f}   [{' '.join(f'{x:.1f}' for x in v)}]")
                print(f"    host->device bytes per window: {int(h2d)} (video block: {bytes_[s]})")
                print(f"    launches on the caller's stream between the copy and fnet's first convolution: {n}  ({names})")
                print(f"    launches on the side stream before cnet's first convolution: {side_n}")
                print(f"    sha256 of disparity + uncertainties: {sums[s]}")
            ma, mb = statistics.median(ms[A]), statistics.median(ms[B])
            print(f"uint8 median / float median = {mb / ma:.4f} ({mb - ma:+.2f} ms); results {'bit-identical' if sums[A] == sums[B] else 'DIFFER'}")
            print()
        print("host: cpus", os.cpu_count(), "loadavg", os.getloadavg())
    finally:
        for s in (A, B):
            s.close()


if __name__ == "__main__":
    main()
