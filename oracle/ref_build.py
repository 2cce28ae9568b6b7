"""Recipe: the reference program as a build product.  TEST INFRASTRUCTURE ONLY.

``build_reference(ref_dir)`` byte-compiles the reference's authoritative module, ``app_dct_svd_single.py``, into
``oracle/_ref/`` and writes a small text file beside it that records the Python version and the SHA-256 of the
source it was made from.  ``oracle/_ref/`` is ignored by git: nothing of the reference's program text is ever
copied into a tracked file.  ``tests/ref_program.py`` loads the compiled module over a stand-in ``cv2``
(``tests/cv2_standin.py``), which is what holds the oracle, the host glue and the drop-in's files to the
reference program itself.

The compiled file is an ordinary ``py_compile`` product (a .pyc in everything but its name).  It is deliberately
not called ``*.pyc``: ignore rules and tree copiers drop Python caches wholesale, and this file is a build
product that has to travel with the tree.

Where the reference tree is absent nothing is touched: a checkout without it builds, tests and benchmarks as
before, and the tests that need the program skip with a reason that names this recipe.

    python -m oracle.ref_build [REFERENCE_DIR]
"""
from __future__ import annotations

import hashlib
import os
import py_compile
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(HERE, "_ref")
SOURCE_NAME = "app_dct_svd_single.py"
COMPILED = os.path.join(REF_OUT, "app_dct_svd_single.bytecode")
INFO = os.path.join(REF_OUT, "app_dct_svd_single.buildinfo.txt")
DEFAULT_REF_DIRS = (os.environ.get("WM_REFERENCE_DIR", ""), "/root/reference")


def find_reference():
    """The directory that holds the reference's source (readable), or None."""
    for d in DEFAULT_REF_DIRS:
        src = os.path.join(d, SOURCE_NAME) if d else ""
        if src and os.path.isfile(src) and os.access(src, os.R_OK):
            return d
    return None


def python_tag() -> str:
    return "%d.%d.%d" % sys.version_info[:3]


def read_info(path: str = INFO) -> dict:
    """The build record as a dict (``python``, ``sha256``, ``source``)."""
    out = {}
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            if "=" in line:
                k, v = line.split("=", 1)
                out[k.strip()] = v.strip()
    return out


def build_reference(ref_dir=None, force: bool = False, out_dir: str = REF_OUT):
    """Compile the reference module into oracle/_ref/ (``out_dir``).  Returns the compiled file's path, or None when
    the reference tree is not there (oracle/_ref/ is then left as it is).  Up to date - same source hash, same
    interpreter - means nothing is rewritten."""
    ref_dir = ref_dir or find_reference()
    if ref_dir is None:
        return None
    compiled = os.path.join(out_dir, os.path.basename(COMPILED))
    info_path = os.path.join(out_dir, os.path.basename(INFO))
    src = os.path.join(ref_dir, SOURCE_NAME)
    with open(src, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    if not force and os.path.exists(compiled) and os.path.exists(info_path):
        info = read_info(info_path)
        if info.get("sha256") == sha and info.get("python") == python_tag():
            return compiled
    os.makedirs(out_dir, exist_ok=True)
    # dfile: the name tracebacks show; the builder's own directory layout does not belong in the product
    py_compile.compile(src, cfile=compiled, dfile=SOURCE_NAME, doraise=True,
                       invalidation_mode=py_compile.PycInvalidationMode.UNCHECKED_HASH)
    with open(info_path, "w", encoding="utf-8") as f:
        f.write(f"source = {SOURCE_NAME}\nsha256 = {sha}\npython = {python_tag()}\n")
    return compiled


if __name__ == "__main__":
    p = build_reference(sys.argv[1] if len(sys.argv) > 1 else None, force=True)
    print(p if p else "reference tree not found; oracle/_ref/ left as it is")
