"""Prints `source sha256` of the gfx950 device assembly of every file in build.SOURCES, compiled with exactly build.FLAGS.

    python tools/isa_digest.py [--keep DIR] [--kernels]

Two trees whose lines are equal have bit-identical device code: the only thing that differs between two compiles of one source
is the per-compile `__hip_cuid_<hash>` symbol, and those lines are dropped before hashing.  Needs hipcc, no GPU.

--kernels prints `source symbol sha256` per kernel instead: the hash of the kernel's text from its label to its .Lfunc_end and of its
.amdhsa_kernel block, normalised (normalise) so that a kernel keeps its hash when it moves to another file or to another place in its file.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppmstereo_amd import build as B  # noqa: E402

_DROPPED = re.compile(r"\s*\.(loc|file|cfi\w*)\b")
_LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp)(\d+)")


def normalise(lines) -> str:
    """The lines of one function without what depends on its place: comments (`;` to the end of the line), empty lines, .loc / .file / .cfi*
    directives and __hip_cuid_ lines go; the function index of .LBB<f>_<n>, .Lfunc_begin<f>, .Lfunc_end<f> becomes a fixed token; .Ltmp<n> is
    numbered by first appearance."""
    tmp = {}

    def local(m):
        kind, num = m.group(1), m.group(2)
        return f".Ltmp{tmp.setdefault(num, len(tmp))}" if kind == "tmp" else f".L{kind}F"

    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip() or _DROPPED.match(ln) or "__hip_cuid_" in ln:
            continue
        out.append(_LOCAL.sub(local, ln))
    return "\n".join(out) + "\n"


def kernel_digests(asm: str) -> dict:
    """{kernel symbol: sha256} of one file of device assembly, in order of appearance.  A kernel is a symbol with an .amdhsa_kernel block."""
    lines = asm.splitlines()
    desc = {}                                                    # symbol -> (first, last) line of its descriptor block
    for i, ln in enumerate(lines):
        w = ln.split()
        if len(w) == 2 and w[0] == ".amdhsa_kernel":
            desc[w[1]] = (i, next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel"))
    out = {}
    for i, ln in enumerate(lines):
        sym = ln.split(":", 1)[0]
        if sym in desc and ln.startswith(sym + ":") and sym not in out:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            d0, d1 = desc[sym]
            body = [x for j, x in enumerate(lines[i:end + 1], i) if not d0 <= j <= d1]      # (llvm puts the block in front of .Lfunc_end)
            out[sym] = hashlib.sha256((normalise(body) + normalise(lines[d0:d1 + 1])).encode()).hexdigest()
    return out


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
            if "--kernels" not in sys.argv:
                print(src, dig)
                continue
            with open(os.path.join(out_dir, src.replace(".hip", ".s"))) as fh:
                for sym, kd in kernel_digests(fh.read()).items():
                    print(src, sym, kd)
