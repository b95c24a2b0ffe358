"""CPU: the drop-in import path.

``models/`` of this repository has NO ``__init__.py`` anywhere: like the reference's ``models/`` it is a PEP 420 namespace portion.  With
this repository in front of the reference on ``sys.path``, ``models.core.{corr,ppmstereo,ppmtereo_update}`` and
``models.core.utils.utils`` bind to the gfx950 implementation while everything else the reference keeps under ``models/`` -- the wrapper
``models/ppm_stereo_model.py`` (its line 12 is the drop-in's import site), ``models.core.extractor``, ``attention``, ``convnext`` ... --
still resolves in the reference.  ``tools/gen_golden.py`` puts the reference FIRST and refuses to run if any module it pins the
oracle with was imported from this repository.

The reference is not part of this repository: the tests below build a stand-in of its ``models/`` layout (the same module paths, empty
files, no ``__init__.py`` at ``models/`` or ``models/core/``) in a temporary directory and check how the two portions resolve against it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# module paths of the reference's models/ namespace that these tests resolve; the last four have same-named modules here
REF_MODULES = ("models/ppm_stereo_model.py", "models/core/extractor.py", "models/core/attention.py", "models/core/convnext.py",
               "models/core/ppmstereo.py", "models/core/corr.py", "models/core/ppmtereo_update.py", "models/core/utils/utils.py")


@pytest.fixture
def ref(tmp_path):
    """A stand-in of the reference's tree: every module of REF_MODULES as an empty file that records where it was imported from."""
    root = tmp_path / "reference"
    for rel in REF_MODULES:
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text("STAND_IN = __file__\n")
    return str(root)


def _run(code, path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=os.pathsep.join(path))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd="/tmp", timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_models_is_a_namespace_portion():
    for d, _, files in os.walk(os.path.join(ROOT, "models")):
        assert "__init__.py" not in files, f"{d}/__init__.py would hide the reference's models namespace"


def test_wrapper_file_and_shim_resolve_side_by_side(ref):
    """models/ppm_stereo_model.py:12 -- found under the reference; its import target -- found here."""
    code = """
import importlib.util as u, os
want = {"models.ppm_stereo_model": %r, "models.core.extractor": %r, "models.core.attention": %r, "models.core.convnext": %r,
        "models.core.ppmstereo": %r, "models.core.corr": %r, "models.core.ppmtereo_update": %r, "models.core.utils.utils": %r}
for name, root in want.items():
    spec = u.find_spec(name)
    assert spec is not None and spec.origin, name
    assert os.path.realpath(spec.origin).startswith(root + os.sep), (name, spec.origin)
from models.core.ppmstereo import PPMStereo            # the line of the wrapper, executed
import ppmstereo_amd.ppmstereo as P
assert PPMStereo is P.PPMStereo
import models.ppm_stereo_model as M                      # the wrapper module itself: the reference's file
assert os.path.realpath(M.STAND_IN).startswith(%r + os.sep)
print("ok")
""" % (ref, ref, ref, ref, ROOT, ROOT, ROOT, ROOT, ref)
    assert "ok" in _run(code, [ROOT, ref])


def test_reference_first_binds_the_reference(ref):
    """The generator's order: the reference in front -> the same names are the reference's own files."""
    code = """
import importlib.util as u, os
for name in ("models.core.ppmstereo", "models.core.corr", "models.core.ppmtereo_update", "models.core.utils.utils"):
    assert os.path.realpath(u.find_spec(name).origin).startswith(%r + os.sep), name
print("ok")
""" % ref
    assert "ok" in _run(code, [ref, ROOT])
