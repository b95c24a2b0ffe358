"""Prints `source sha256` of the gfx950 device assembly of every file in build.SOURCES, compiled with exactly build.FLAGS.

    python tools/isa_digest.py [--keep DIR]

Two trees whose lines are equal have bit-identical device code: the only thing that differs between two compiles of one source
is the per-compile `__hip_cuid_<hash>` symbol, and those lines are dropped before hashing.  Needs hipcc, no GPU.
"""
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppmstereo_amd import build as B  # noqa: E402


def digest(src: str, out_dir: str) -> str:
    asm = os.path.join(out_dir, src.replace(".hip", ".s"))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + B.FLAGS + ["--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", asm], check=True, stderr=subprocess.DEVNULL)
    with open(asm, "rb") as fh:
        return hashlib.sha256(b"".join(ln for ln in fh if b"__hip_cuid_" not in ln)).hexdigest()


if __name__ == "__main__":
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(4) as pool:
        out_dir = keep or tmp
        os.makedirs(out_dir, exist_ok=True)
        for src, dig in zip(B.SOURCES, pool.map(lambda s: digest(s, out_dir), B.SOURCES)):
            print(src, dig)
