"""The fixtures of tests/golden/webp_lossy_dec (written by webp_vp8_dec_cases.py) for the lossy WebP decoder's tests: every
p_ (Pillow-encoded), h_ (hand-written) and s_ (the kernels' seams) file with the B,G,R,A frame Pillow's libwebp gives for
it, the refused (r_) and damaged (d_) files, and the truncated files with Pillow's recorded verdicts."""
import functools
import json
import os

import numpy as np

import webp_vp8_dec_cases as cases

HERE = cases.HERE
IMP_OK, IMP_ERROR_UNSUPPORTED, IMP_ERROR_MALLOC_FAILED, IMP_ERROR_DECODE_FAILED = 0, 1, 2, 3
ACCEPT_LOSSY = 1


def read(name):
    with open(os.path.join(HERE, name), "rb") as f:
        return f.read()


def bgra(rgb):
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[:, :, :3] = rgb[:, :, ::-1]
    return out


@functools.lru_cache(maxsize=None)
def load():
    """[(name, file bytes, expected HxWx4 array)] in name order"""
    exp = np.load(os.path.join(HERE, "expected.npz"))
    return [(f[:-5], read(f), bgra(exp[f[:-5]])) for f in sorted(os.listdir(HERE)) if f.endswith(".webp") and f[:2] in ("p_", "h_", "s_")]


def refused():
    """[(name, file bytes)]: IMP_ERROR_UNSUPPORTED"""
    return [(f[:-5], read(f)) for f in sorted(os.listdir(HERE)) if f.startswith("r_")]


def damaged():
    """[(name, file bytes)]: IMP_ERROR_DECODE_FAILED"""
    return [(f[:-5], read(f)) for f in sorted(os.listdir(HERE)) if f.startswith("d_")]


@functools.lru_cache(maxsize=None)
def truncated():
    """[(label, file bytes, Pillow decoded it, to the fixture's frame, fixture name)]"""
    with open(os.path.join(HERE, "verdicts.json")) as f:
        verdicts = json.load(f)
    return [("%s-%d-%s" % (name, n, where), cases.cut(read(name + ".webp"), n, where), ok, same, name) for name, n, where, ok, same in verdicts]
