"""glue/ (SURVEY 8f N3): the nginx-side binding as source.  It cannot be BUILT here (nginx / OpenCV / FreeImage headers and
libraries are absent).  What the suite checks without a checkout of the reference is that the glue calls nothing the C ABI
headers do not declare.  That glue/apply_glue.sh applies to the reference revision it names and that the patched module
COMPILES against tests/c/decls/ needs the reference's own sources, which this repository does not carry: run
`python glue/check_glue.py <reference checkout>` for that."""
import os

from conftest import ROOT


def test_glue_uses_only_declared_abi_symbols():
    import re

    src = open(os.path.join(ROOT, "glue", "imp_gpu_bridge.c")).read()
    header = open(os.path.join(ROOT, "include", "impgpu.h")).read()
    header += open(os.path.join(ROOT, "include", "impgpu_broker.h")).read()
    used = set(re.findall(r"\b(impgpu_[a-z0-9_]+)\s*\(", src))
    declared = set(re.findall(r"\b(impgpu_[a-z0-9_]+)\s*\(", header))
    assert used and used <= declared, used - declared
