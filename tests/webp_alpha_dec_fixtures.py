"""The fixtures of tests/golden/webp_alpha_dec (written by webp_alpha_dec_cases.py) for the tests of the lossy WebP decoder's
alpha route: every p_ (Pillow-written) and h_ (hand-assembled) file with the B,G,R,A frame Pillow's libwebp gives for it as
mode RGBA, the refused (r_) and damaged (d_) files, and the files whose ALPH payload was cut, with Pillow's verdicts."""
import functools
import json
import os

import numpy as np

import webp_alpha_dec_cases as cases

HERE = cases.HERE
IMP_OK, IMP_ERROR_UNSUPPORTED, IMP_ERROR_MALLOC_FAILED, IMP_ERROR_DECODE_FAILED = 0, 1, 2, 3
ACCEPT_LOSSY, ACCEPT_ALPHA = 1, 2
ACCEPT = ACCEPT_LOSSY | ACCEPT_ALPHA
FILTERS = cases.FILTERS


def read(name):
    with open(os.path.join(HERE, name), "rb") as f:
        return f.read()


def bgra(rgba):
    return np.ascontiguousarray(rgba[:, :, [2, 1, 0, 3]])


@functools.lru_cache(maxsize=None)
def load():
    """[(name, file bytes, expected HxWx4 B,G,R,A array)] in name order"""
    exp = np.load(os.path.join(HERE, "expected.npz"))
    return [(f[:-5], read(f), bgra(exp[f[:-5]])) for f in sorted(os.listdir(HERE)) if f.endswith(".webp") and f[:2] in ("p_", "h_")]


def get(name):
    return [x for x in load() if x[0] == name][0]


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
    return [("%s-%d" % (name, n), cases.cut_alph(read(name + ".webp"), n), ok, same, name) for name, n, ok, same in verdicts]


def alph_header(blob):
    """the ALPH chunk's header byte, or None"""
    p = cases.find_chunk(blob, b"ALPH")
    return p[0] if p else None
