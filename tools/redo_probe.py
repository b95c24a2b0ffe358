"""How many 256-query tiles of the rescale-free attention kernel go to its fix-up pass (a score more than 2^16 -- fp16 P~ -- above the query's softmax
reference) on the synthetic inputs of the BASELINE configurations?  usage: tools/redo_probe.py [T H W iters]   (GPU box)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ppmstereo_amd import weights as Wm
from ppmstereo_amd.ppmstereo import PPMStereoHotPath
from ppmstereo_amd.synth import synth_cascade_feats
T, H, W, iters = (int(x) for x in sys.argv[1:5]) if len(sys.argv) > 4 else (5, 320, 512, 10)
dev = torch.device("cuda:0")
model = PPMStereoHotPath().load_hot_path_weights(Wm.hot_path_weights()).to(dev).eval()
feats = {k: v.to(dev) for k, v in synth_cascade_feats(T, H, W).items()}
diag = {}
model.cascade(feats, iters, T, test_mode=True, diagnostics=diag)
for scale, h in diag["attn_redo"].items():
    print(f"T={T} {H}x{W} iters={iters} scale {scale}: {h['calls']} attention calls, {h['tiles']} tiles, {h['flagged']} handed to the fix-up pass")
