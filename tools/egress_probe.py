"""Same-box A/B of the back door: PPMStereo.forward_batch_test on a float32 host video with output=None (tree A, --parent DIR: a checkout of the
parent commit with its library built; default: this tree, whose default path is the parent's) against this tree's with
output=OutputSpec(disparity="u16", uncertainty="u8").
    python tools/egress_probe.py --parent DIR [--runs 12] [--windows] > profiles/rNN_egress_ab.txt
Two worker processes (one per tree) stay alive and take turns, one whole call each, so both see the same box, clocks and host load.  Per side:
median / min / max whole-call ms (host video -> host results), the device->host bytes of a call, and what is enqueued behind the last convex
upsampling of a one-window call (library launches and torch ops that launch; counted in one extra call after the timed ones, with Python-level
hooks that the timed calls never see).  Config 2: T = 5, 320x512, iters = 10 (one window); --windows adds T = 30 at kernel_size = 20 (three
windows through the ClipPipeline: only kept frames cross on side B).  The bar: B's median is not above A's by more than the
+-2 % same-box spread.
    python tools/egress_probe.py --points [--runs 12]
The point-cloud A/B, both sides on this tree and on a uint8 video that lies on the device: A = forward(test_mode=True), then the same arithmetic
in torch on the device (OutputSpec.reference on the float32 results) and the cloud's copy to the host; B = forward(..., output=spec) -- "xyz" f32
points with both gates, from the one ppms_scene_egress launch -- and the same copy.  The two clouds are compared bit for bit (NaN = NaN).
    python tools/egress_probe.py --cloud [--runs 12]
The compact-cloud A/B, both sides on this tree, on the same device video and with the same gates: A = forward(..., output=spec with points), then
pts[valid] in torch on the device and that tensor's copy to the host; B = forward(..., output=spec with cloud) -- ppms_cloud_egress's two launches
behind the planes' one --, the counts' copy to the host and then count records per frame.  The two compact clouds are compared bit for bit, and
the valid fraction of the pixels is printed with the times: the bytes B saves are that fraction's complement, the times are what this run
measured on this video and nothing more.
    python tools/egress_probe.py --colour [--runs 12]
The coloured-cloud A/B, both sides on this tree with colour="bgra8": A = the "xyz" cloud with its indices, then rgba.view(-1)[cloud_index] in torch
on the device, joined to the records, and their copy to the host; B = cloud_layout="xyzrgb" (ppms_cloud_egress_colour), colour_plane=False, and
the same copy.  The records are compared as int32 words.  No claim rests on its times."""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ("ppms_convex_upsample", "ppms_convex_upsample_3d", "ppms_bilinear", "ppms_disparity_egress", "ppms_scene_egress", "ppms_cloud_egress",
            "ppms_cloud_egress_colour", "ppms_normals_egress", "ppms_cloud_egress_normals")


# ------------------------------------------------------------------------------------------------------------------------------ worker
def worker(tree: str, side: str):
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
    kw = {"output": P.OutputSpec(disparity="u16", uncertainty="u8")} if side == "egress" else {}
    say = lambda *a: print(*a, flush=True)
    state = {}

    def setup(T, H, W, iters):
        state["video"] = Wm.hash_uniform((T, 2, 3, H, W), 613, 0.0, 255.0).round().contiguous()
        state["call"] = lambda: m.forward_batch_test({"stereo_video": state["video"]}, kernel_size=20, iters=iters, **kw)
        if side.startswith("points"):
            spec = P.OutputSpec(uncertainty=None, points="f32", Q=P.OutputSpec.q_matrix(721.5377, 0.54, W / 2, H / 2), max_uncertainty=0.5, max_depth=50.0)
            i1, i2 = (state["video"][:, k][None].to(torch.uint8).to(dev) for k in (0, 1))
            if side == "points":
                state["call"] = lambda: {"points": m.forward(i1, i2, iters=iters, test_mode=True, output=spec)["points"].cpu()}
            else:
                state["call"] = lambda: {"points": spec.reference(*m.forward(i1, i2, iters=iters, test_mode=True))["points"].cpu()}
        if side.startswith("cloud"):                     # (the compact cloud under the key "points": one (records, 3) tensor, frame after frame)
            gates = dict(uncertainty=None, Q=P.OutputSpec.q_matrix(721.5377, 0.54, W / 2, H / 2), max_uncertainty=0.5, max_depth=50.0)
            i1, i2 = (state["video"][:, k][None].to(torch.uint8).to(dev) for k in (0, 1))
            if side == "cloud":
                spec = P.OutputSpec(cloud="f32", **gates)

                def call():
                    out = m.forward(i1, i2, iters=iters, test_mode=True, output=spec)
                    counts = out["cloud_counts"][0].cpu().tolist()
                    return {"points": torch.cat([out["cloud"][0, f, :c].cpu() for f, c in enumerate(counts)])}
            else:
                spec = P.OutputSpec(points="f32", **gates)

                def call():
                    pts = m.forward(i1, i2, iters=iters, test_mode=True, output=spec)["points"][0]
                    return {"points": pts[~pts[..., 2].isnan()].cpu()}
            state["call"] = call
        if side.startswith("colour"):                    # (the coloured cloud under the key "points": one int32 (records, 4) tensor of words, frame after frame)
            gates = dict(uncertainty=None, colour="bgra8", cloud="f32", Q=P.OutputSpec.q_matrix(721.5377, 0.54, W / 2, H / 2), max_uncertainty=0.5, max_depth=50.0)
            i1, i2 = (state["video"][:, k][None].to(torch.uint8).to(dev) for k in (0, 1))
            if side == "colour":
                spec = P.OutputSpec(cloud_layout="xyzrgb", colour_plane=False, **gates)

                def call():
                    out = m.forward(i1, i2, iters=iters, test_mode=True, output=spec)
                    counts = out["cloud_counts"][0].cpu().tolist()
                    return {"points": torch.cat([out["cloud"][0, f, :c].cpu() for f, c in enumerate(counts)]).view(torch.int32)}
            else:
                spec = P.OutputSpec(cloud_index=True, **gates)

                def call():
                    out = m.forward(i1, i2, iters=iters, test_mode=True, output=spec)
                    counts = out["cloud_counts"][0].cpu().tolist()
                    words = out["colour"][0].view(torch.int32).flatten(1)
                    recs = [torch.cat([out["cloud"][0, f, :c].view(torch.int32), words[f][out["cloud_index"][0, f, :c].long()][:, None]], dim=1).cpu()
                            for f, c in enumerate(counts)]
                    return {"points": torch.cat(recs)}
            state["call"] = call
        for _ in range(3):
            state["call"]()
        torch.cuda.synchronize()

    def count():
        """One call with hooks: device->host bytes, and every library launch of LAUNCHES / torch op with a device or host result behind the
        last convex upsampling."""
        from torch.utils._python_dispatch import TorchDispatchMode
        events, d2h = [], [0]

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                name = func._schema.name
                view = any(r.alias_info is not None and not r.alias_info.is_write for r in func._schema.returns)
                tensors = [a for a in args if torch.is_tensor(a)]
                if name == "aten::copy_" and len(tensors) == 2 and tensors[1].is_cuda and not tensors[0].is_cuda:
                    d2h[0] += tensors[1].numel() * tensors[1].element_size()
                    events.append("d2h:copy_")
                elif name == "aten::_to_copy" and tensors and tensors[0].is_cuda and torch.is_tensor(out) and not out.is_cuda:
                    d2h[0] += tensors[0].numel() * tensors[0].element_size()
                    events.append("d2h:_to_copy")
                elif not view and torch.is_tensor(out) and not name.startswith(("aten::empty", "aten::new_empty")):
                    events.append(("gpu:" if out.is_cuda else "host:") + name.replace("aten::", ""))
                return out

        lib = L.load()
        for name in LAUNCHES:
            if hasattr(lib, name):
                fn = getattr(lib, name)
                setattr(lib, name, (lambda fn, name: lambda *a: (events.append("lib:" + name), fn(*a))[1])(fn, name))
        with Mode():
            state["call"]()
        last = max((i for i, e in enumerate(events) if e.startswith("lib:ppms_convex_upsample")), default=-1)
        tail = events[last + 1:]
        say("count", d2h[0], sum(e.startswith(("lib:", "gpu:")) for e in tail), sum(e.startswith("host:") for e in tail), ",".join(tail))

    for line in sys.stdin:
        cmd = line.split()
        if not cmd:
            continue
        if cmd[0] == "setup":
            setup(*map(int, cmd[1:5]))
            say("ready", state["video"].numel() * state["video"].element_size())
        elif cmd[0] == "run":
            t0 = time.perf_counter()
            state["out"] = state["call"]()
            say("ms", f"{1e3 * (time.perf_counter() - t0):.3f}")
        elif cmd[0] == "shape":
            o = state["out"]
            say("shape", ";".join(f"{k}:{str(v.dtype).replace('torch.', '')}{list(v.shape)}".replace(" ", "") for k, v in o.items() if torch.is_tensor(v)))
        elif cmd[0] == "digest":
            import hashlib
            pts = state["out"]["points"]                 # (float points: NaN = NaN; the coloured cloud's int32 words as they are)
            say("digest", hashlib.sha256((pts.nan_to_num(nan=-1.0) if pts.is_floating_point() else pts).numpy().tobytes()).hexdigest()[:16])
        elif cmd[0] == "count":
            count()
        elif cmd[0] == "quit":
            break


# ------------------------------------------------------------------------------------------------------------------------------ driver
class Side:
    def __init__(self, label, tree, side):
        self.label = label
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", side, "--tree", tree], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(self, *cmd):
        self.p.stdin.write(" ".join(map(str, cmd)) + "\n")
        self.p.stdin.flush()
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"worker '{self.label}' ended (exit {self.p.wait()})")
            parts = line.split()
            if parts and parts[0] in ("ready", "ms", "shape", "count", "digest"):
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
    ap.add_argument("--parent", default=None, help="tree of the parent commit with its libppms.so built (default: this tree's default path)")
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--windows", action="store_true", help="also T = 30 at kernel_size = 20: three windows through the ClipPipeline")
    ap.add_argument("--points", action="store_true", help="the point-cloud A/B instead: the reprojection in torch on the device against ppms_scene_egress")
    ap.add_argument("--cloud", action="store_true", help="the compact-cloud A/B instead: organised points and pts[valid] in torch against ppms_cloud_egress")
    ap.add_argument("--colour", action="store_true", help='the coloured-cloud A/B instead: "xyz" records, indices and a gather of the colour plane in torch against "xyzrgb"')
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=HERE)
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.tree), a.worker)
    ptree = os.path.abspath(a.parent) if a.parent else HERE
    if a.colour:
        A = Side('forward(output=OutputSpec(colour="bgra8", cloud="f32", cloud_index=True, ...)), rgba.view(-1)[cloud_index] on the device, records -> host', HERE, "colour_torch")
        B = Side('forward(output=OutputSpec(colour="bgra8", cloud="f32", cloud_layout="xyzrgb", colour_plane=False, ...)), counts -> host, count records per frame -> host',
                 HERE, "colour")
        a.cloud = True                                   # (from here on: the compact cloud's report)
    elif a.cloud:
        A = Side('forward(output=OutputSpec(points="f32", Q=..., max_uncertainty=0.5, max_depth=50)), pts[valid] on the device -> host', HERE, "cloud_torch")
        B = Side('forward(output=OutputSpec(cloud="f32", Q=..., max_uncertainty=0.5, max_depth=50)), counts -> host, count records per frame -> host', HERE, "cloud")
    elif a.points:
        A = Side("forward(), then OutputSpec.reference in torch on the device, points -> host", HERE, "points_torch")
        B = Side('forward(output=OutputSpec(points="f32", Q=..., max_uncertainty=0.5, max_depth=50)), points -> host', HERE, "points")
    else:
        A = Side("output=None, " + ("parent commit's tree" if a.parent else "this tree (default path as in the parent)"), ptree, "default")
        B = Side('output=OutputSpec(disparity="u16", uncertainty="u8"), this tree', HERE, "egress")
    try:
        for T, H, W, iters, runs in [(5, 320, 512, 10, a.runs)] + ([(30, 320, 512, 10, max(3, a.runs // 3))] if a.windows else []):
            for s in (A, B):
                s.ask("setup", T, H, W, iters)
            ms = {A: [], B: []}
            for _ in range(runs):
                for s in (A, B):                                # alternate: one whole call each
                    ms[s].append(float(s.ask("run")[0]))
            what = "forward(device uint8 video) -> host points" if a.points or a.cloud else "forward_batch_test(host video) -> host results"
            print(f"== T = {T}, {H}x{W}, iters = {iters}, kernel_size = 20: {what}, {runs} alternating calls per side")
            for s in (A, B):
                v = ms[s]
                shape = s.ask("shape")[0]
                d2h, n_dev, n_host, names = (s.ask("count") + [""])[:4]
                print(f"{s.label}:")
                print(f"    whole call ms: median {statistics.median(v):.2f}  min {min(v):.2f}  max {max(v):.2f}   [{' '.join(f'{x:.1f}' for x in v)}]")
                print(f"    results: {shape}")
                print(f"    device->host bytes per call: {int(d2h)} ({int(d2h) / (T * H * W):.2f} per pixel and frame of the video)")
                print(f"    behind the last convex upsampling: {n_dev} device launches / copies, {n_host} host torch ops  ({names})")
            ma, mb = statistics.median(ms[A]), statistics.median(ms[B])
            print(f"egress median / default median = {mb / ma:.4f} ({mb - ma:+.2f} ms)")
            if a.points or a.cloud:
                da, db = A.ask("digest")[0], B.ask("digest")[0]
                print(f"points digest A {da}  B {db}: {'bit-identical' if da == db else 'DIFFERENT'}")
            if a.cloud:
                records = int(B.ask("shape")[0].split("[")[1].split(",")[0])
                print(f"valid fraction: {records} of {T * H * W} pixels = {records / (T * H * W):.4f}")
            print()
        print("host: cpus", os.cpu_count(), "loadavg", os.getloadavg())
    finally:
        for s in (A, B):
            s.close()


if __name__ == "__main__":
    main()
