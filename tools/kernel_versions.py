"""The launch plan of the convolutions: which kernel serves which launch, with what descriptor and weights.  Per scale of the update blocks
(and with --encoders, per launch of fnet / cnet / the SST block at the same geometry): a summary by kernel, then one line per launch --
kernel, K slices, tile hint, y sweep, the descriptor's non-pointer fields (pointers as 1 / 0: set or null) and a digest of the packed weight
and bias bytes.  Reads public attributes only, so two trees' plans can be compared line for line.
usage: tools/kernel_versions.py [T H W] [--encoders]   (GPU box)"""
import collections, ctypes as C, hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ppmstereo_amd import weights as Wm
from ppmstereo_amd.convplan import KERNEL_NAMES as names
from ppmstereo_amd.engine import ConvOp
from ppmstereo_amd.ppmstereo import PPMStereoHotPath
args = [a for a in sys.argv[1:] if not a.startswith("--")]
T, H, W = (int(x) for x in args[:3]) if len(args) >= 3 else (5, 320, 512)
dev = torch.device("cuda:0")


def fields(s):
    """Non-pointer fields of a ctypes structure, flattened (pointers: 1 set / 0 null)."""
    out = []
    for f, ty in s._fields_:
        v = getattr(s, f)
        if isinstance(v, C.Structure):
            out += [f"{f}.{x}" for x in fields(v)]
        elif isinstance(v, C.Array):
            for i, e in enumerate(v):
                out += [f"{f}[{i}].{x}" for x in fields(e)]
        elif ty is C.c_void_p:
            out.append(f"{f}={int(v is not None)}")
        else:
            out.append(f"{f}={v:.9g}" if isinstance(v, float) else f"{f}={v}")
    return out


def digest(op, p):
    t = next((t for t in op.keep if torch.is_tensor(t) and t.data_ptr() == p), None)
    return "-" if t is None else hashlib.sha1(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def report(title, ops):
    by = collections.defaultdict(list)
    for k, op in ops.items():
        by[names[op.version] + (" (K-sliced + reduce)" if op.nslice > 1 else "")].append(k)
    print(title)
    for v, ks in sorted(by.items()):
        print(f"   {v:32s} {len(ks):3d}: {' '.join(sorted(ks))}")
    for k in sorted(ops):
        op = ops[k]
        print(f"   | {k:12s} {names[op.version]:12s} nslice={op.nslice} wm={op.wm_hint} ysweep={int(bool(op.ysweep))} w={digest(op, op.desc.w)} "
              f"bias={digest(op, op.desc.bias)} {' '.join(fields(op.desc))}")


model = PPMStereoHotPath().load_hot_path_weights(Wm.hot_path_weights()).to(dev).eval()
for s, blk in ((16, model.update_block16), (8, model.update_block08), (4, model.update_block04)):
    eng = blk.engine(T, H // s, W // s, dev)
    report(f"T={T} {H}x{W} scale 1/{s} ({H // s}x{W // s}):", {k: op for k, op in eng.op.items() if isinstance(op, ConvOp)})

if "--encoders" in sys.argv:
    # the engines of fnet (2T images), cnet (T images) and the SST block (1/16 features), built by one call each
    from ppmstereo_amd.cnet import Feature
    from ppmstereo_amd.encoder import BasicEncoder
    from ppmstereo_amd.sst import SSTBlock
    fnet, cnet, sst = BasicEncoder(256, "instance"), Feature("tiny", 256), SSTBlock()
    fnet.load_state_dict(Wm.fnet_weights()), cnet.load_state_dict(Wm.cnet_weights()), sst.load_state_dict(Wm.sst_weights())
    fnet, cnet, sst = fnet.to(dev).eval(), cnet.to(dev).eval(), sst.to(dev).eval()
    img = torch.zeros(T, 3, H, W, device=dev)
    with torch.no_grad():
        fnet([img, img]), cnet(img), sst(torch.zeros(T, 256, H // 16, W // 16, device=dev), torch.zeros(T, 256, H // 16, W // 16, device=dev), T)
    torch.cuda.synchronize()
    for tag, mod, steps in (("fnet", fnet, lambda e: [op for _, op in e.ops]), ("cnet", cnet, lambda e: e.steps), ("sst", sst, lambda e: e.steps)):
        for eng in mod._engines.values():
            report(f"{tag} T={T} {H}x{W}:", {f"{i:03d}": op for i, op in enumerate(steps(eng)) if isinstance(op, ConvOp)})
