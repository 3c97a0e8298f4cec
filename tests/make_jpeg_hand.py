"""Generates tests/golden/jpeg_hand/: baseline JPEG files written by hand (jpeg_writer.py) from coefficients no encoder
of 8-bit photographs produces, Pillow's pixels for them (expected.npz) and manifest.json.

    python tests/make_jpeg_hand.py            # rewrites the folder; deterministic, byte for byte
    python tests/make_jpeg_hand.py --check    # compares with the committed folder instead

The tests import cases() / build() from here to get the coefficients every file was WRITTEN from (regenerated from the
seed, checked by the manifest's sha256) -- not what some decoder read back.

For every in-domain file (jpeg_writer.idct_domain) the generator asserts that orc.jpeg_decode equals Pillow.  If that
ever fails the domain rule is wrong: correct the rule, do not loosen it per file.  The out-of-domain files get no
expected pixels: libjpeg-turbo's SIMD IDCT, plain-C libjpeg and a 32-bit IDCT with saturation give three answers there.
"""
import hashlib
import io
import json
import os
import sys
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_writer as jw  # noqa: E402

OUT = os.path.join(HERE, "golden", "jpeg_hand")
SUBS = ["gray", "4:4:4", "4:2:2", "4:4:0", "4:2:0"]
TAG = {"gray": "gray", "4:4:4": "444", "4:2:2": "422", "4:4:0": "440", "4:2:0": "420"}
UNSUPPORTED = 1                                          # IMP_ERROR_UNSUPPORTED, the deferred file's verdict


def rng_of(name):
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


def flat(v):
    return np.full(64, v, dtype=np.int64)


def fit(plane, q):
    """halves the coefficients of every out-of-domain block until it is in-domain"""
    plane = plane.copy()
    for _ in range(12):
        a, b, _ = jw.idct_domain(plane, q)
        bad = (a > jw.DOMAIN_LIMIT) | (b > jw.DOMAIN_LIMIT)
        if not bad.any():
            return plane
        plane[bad] = np.trunc(plane[bad] / 2).astype(plane.dtype)
    raise AssertionError("a block does not fit the domain")


def textured(rng, shape, dc=100, nac=6, ac=30, reach=20):
    """picture-like blocks: a DC term and a few low-frequency AC terms (zig-zag positions below `reach`)"""
    p = np.zeros(shape + (64,), dtype=np.int64)
    p[:, :, 0] = rng.integers(-dc, dc + 1, shape)
    for _ in range(nac):
        k = rng.integers(1, reach, shape)
        v = rng.integers(-ac, ac + 1, shape)
        for by in range(shape[0]):
            for bx in range(shape[1]):
                p[by, bx, jw.ZIGZAG[k[by, bx]]] = v[by, bx]
    return p


# ---------------------------------------------------------------- the families
def colour_rule():
    out = []
    ids = {"ids123": (1, 2, 3), "ids012": (0, 1, 2), "idsRGB": (ord("R"), ord("G"), ord("B"))}
    marks = {"jfif": dict(jfif=True), "none": dict(jfif=False), "adobe0": dict(jfif=False, adobe=0), "adobe1": dict(jfif=False, adobe=1),
             "adobe2": dict(jfif=False, adobe=2), "jfif_adobe0": dict(jfif=True, adobe=0)}
    for sub in ("4:4:4", "4:2:0"):
        for iname, idv in ids.items():
            for mname, mk in marks.items():
                name = "col_%s_%s_%s" % (TAG[sub], iname, mname)
                ycc = True if mk["jfif"] else (mk["adobe"] != 0 if mk.get("adobe") is not None else iname != "idsRGB")

                def make(name=name, sub=sub, idv=idv, mk=mk):
                    rng = rng_of(name)
                    comps = jw.components(sub, idv)
                    w, h = (23, 17) if sub == "4:4:4" else (37, 19)
                    q = {0: flat(8), 1: flat(11)}
                    _, _, shapes = jw.geometry(w, h, comps)
                    planes = [fit(textured(rng, s, dc=110), q[c[3]]) for s, c in zip(shapes, comps)]
                    return dict(width=w, height=h, comps=comps, qtabs=q, planes=planes, **mk)
                out.append(dict(name=name, family="colour", make=make, ycc=ycc))
    return out


def tables_family():
    out = []
    natural = np.arange(1, 65, dtype=np.int64)

    def simple(name, sub, q, tq=(0, 1, 1), w=41, h=23, **kw):
        def make():
            rng = rng_of(name)
            comps = jw.components(sub, tq=tq)
            _, _, shapes = jw.geometry(w, h, comps)
            planes = [fit(textured(rng, s, dc=300, ac=120, reach=40), q[c[3]]) for s, c in zip(shapes, comps)]
            return dict(width=w, height=h, comps=comps, qtabs=q, planes=planes, **kw)
        return dict(name=name, family="tables", make=make)

    out.append(simple("tab_420_three_q", "4:2:0", {0: flat(3), 1: natural, 2: flat(255)}, tq=(0, 1, 2)))
    out.append(simple("tab_420_three_q_one_dqt", "4:2:0", {0: flat(255), 1: flat(3), 2: natural}, tq=(2, 0, 1), one_dqt=True, one_dht=True))
    for sof in (0xC0, 0xC1):
        for qv in (3, 700):
            out.append(simple("tab_420_pq1_q%d_sof%d" % (qv, sof & 1), "4:2:0", {0: flat(qv), 1: natural * (qv // 3)}, pq=1, sof=sof))
    out.append(simple("tab_444_pq_mixed", "4:4:4", {0: flat(5), 1: flat(300)}, pq={0: 0, 1: 1}, sof=0xC1))
    for k, sel in enumerate(([(1, 1), (0, 0), (0, 0)], [(0, 1), (1, 0), (0, 0)], [(0, 0), (0, 0), (0, 0)], [(1, 0), (0, 1), (1, 1)])):
        out.append(simple("tab_420_sel%d" % k, "4:2:0", {0: flat(6), 1: natural}, tables=sel))
        out.append(simple("tab_422_sel%d" % k, "4:2:2", {0: natural, 1: flat(9)}, tables=sel, dri=2))
    out.append(simple("tab_gray_table1", "gray", {2: flat(7)}, tq=(2,), tables=[(1, 1)]))
    d = simple("tab_444_three_huffman", "4:4:4", {0: flat(6), 1: flat(10)}, tables=[(0, 0), (1, 1), (2, 2)])
    d["verdict"] = UNSUPPORTED                           # three different tables: the product leaves the file to the host decoder
    out.append(d)
    d = simple("tab_420_three_dc_tables", "4:2:0", {0: flat(6), 1: flat(10)}, tables=[(0, 0), (1, 1), (2, 1)])
    d["verdict"] = UNSUPPORTED
    out.append(d)
    return out


SINGLE = [1023, -1023, 512, -512, 511]


def symbols_family():
    out = []
    at = 0                                               # the family's running block number: which AC term a 'cat' block carries
    for sub in SUBS:
        w, h = {"gray": (40, 24), "4:4:4": (33, 17), "4:2:2": (40, 24), "4:4:0": (31, 33), "4:2:0": (72, 40)}[sub]
        for kind in ("cat", "runs", "long"):
            for dri, fill in ((0, 0), (1, 0), (5, 0), (1, 2), (5, 2)):
                name = "sym_%s_%s_dri%d%s" % (TAG[sub], kind, dri, "_fill" if fill else "")
                comps = jw.components(sub)
                _, _, shapes = jw.geometry(w, h, comps)
                first = at
                if kind == "cat":
                    at += sum(s[0] * s[1] for s in shapes)

                def make(name=name, kind=kind, comps=comps, shapes=shapes, w=w, h=h, dri=dri, fill=fill, first=first):
                    rng = rng_of(name)
                    q = {0: flat(1), 1: flat(1)}
                    kw = {}
                    planes = []
                    n = first
                    for s in shapes:
                        p = np.zeros(s + (64,), dtype=np.int64)
                        for by in range(s[0]):
                            for bx in range(s[1]):
                                if kind == "cat":        # DC swings of category 11, one AC term of category 10 / 9 per block
                                    p[by, bx, 0] = 1023 if (by * s[1] + bx) % 2 else -1023
                                    p[by, bx, jw.ZIGZAG[n % 63 + 1]] = SINGLE[n % 5]
                                    n += 1
                                elif kind == "runs":     # ZRL x 3 + coefficient 63, blocks without EOB, all-zero blocks
                                    pick = int(rng.integers(0, 4))
                                    p[by, bx, 0] = int(rng.integers(-60, 61))
                                    if pick == 0:
                                        p[by, bx, 63] = int(rng.choice([-3, -1, 1, 2, 77]))
                                    elif pick == 1:
                                        p[by, bx, 1:] = rng.integers(-2, 3, 63)
                                        p[by, bx, 63] = int(rng.choice([-1, 1]))
                                    elif pick == 2:
                                        p[by, bx, jw.ZIGZAG[17]] = 5
                                        p[by, bx, jw.ZIGZAG[50]] = -9
                                        p[by, bx, 63] = 1
                                    else:
                                        p[by, bx, 0] = 0
                                else:                    # many symbols, so that the skewed tables have a long tail that is used
                                    p[by, bx, 0] = int(rng.integers(-1023, 1024)) >> int(rng.integers(0, 11))
                                    for _ in range(int(rng.integers(0, 9))):
                                        p[by, bx, int(rng.integers(1, 64))] = int(rng.integers(-255, 256)) >> int(rng.integers(0, 8))
                        planes.append(p)
                    if kind == "long":
                        keys = [("dc", 0), ("ac", 0)] + ([("dc", 1), ("ac", 1)] if len(comps) == 3 else [])
                        kw = dict(skew=keys, extra={k: (list(range(16)) if k[0] == "dc" else [0xFA, 0xE9, 0xD8]) for k in keys})
                    return dict(width=w, height=h, comps=comps, qtabs=q, planes=planes, dri=dri, fill=fill, **kw)
                out.append(dict(name=name, family="symbols", make=make, kind=kind, first=first))
    return out


def row0_block(amp, signs):
    """a block whose only terms are the eight of its first row: every column's pass-1 output is 4 * amp * q, and the row
    pass adds them up far past the sample range"""
    b = np.zeros(64, dtype=np.int64)
    b[:8] = amp * np.asarray(signs)
    return b


def saturation_family():
    out = []

    def sparse(name, sub, w, h):
        def make():
            rng = rng_of(name)
            comps = jw.components(sub)
            q = {0: flat(16), 1: flat(13)}
            _, _, shapes = jw.geometry(w, h, comps)
            planes = []
            for s, c in zip(shapes, comps):
                p = np.zeros(s + (64,), dtype=np.int64)
                for by in range(s[0]):
                    for bx in range(s[1]):
                        pick = (by * s[1] + bx) % 4
                        if pick == 0:                    # the eight terms of the first row: past +-2000
                            p[by, bx] = row0_block(int(rng.integers(150, 250)), rng.choice([-1, 1], 8))
                        else:                            # sparse large terms anywhere, kept only while the block stays in-domain
                            for _ in range(int(rng.integers(2, 7))):
                                trial = p[by, bx].copy()
                                trial[int(rng.integers(0, 64))] = int(rng.integers(-1023, 1024))
                                if jw.in_domain(trial, q[c[3]]):
                                    p[by, bx] = trial
                planes.append(p)
            return dict(width=w, height=h, comps=comps, qtabs=q, planes=planes)
        return dict(name=name, family="saturation", make=make)

    out += [sparse("sat_gray_sparse", "gray", 72, 40), sparse("sat_444_sparse", "4:4:4", 40, 24), sparse("sat_420_sparse", "4:2:0", 64, 32),
            sparse("sat_440_sparse", "4:4:0", 24, 40)]

    def alternating(name, sub, w, h):
        def make():
            rng = rng_of(name)
            comps = jw.components(sub)
            q = {0: flat(16), 1: flat(4)}
            _, _, shapes = jw.geometry(w, h, comps)
            planes = []
            for ci, s in enumerate(shapes):
                p = np.zeros(s + (64,), dtype=np.int64)
                for by in range(s[0]):
                    for bx in range(s[1]):
                        if ci == 0:                      # saturated luma: 0 or 255 all over the block
                            p[by, bx, 0] = 250 if (by + bx) % 2 else -250
                        else:                            # the highest horizontal frequency: 0, 255, 0, 255 ... from sample to sample
                            p[by, bx, 7] = int(rng.choice([-1000, 1000]))
                            if (by + bx + ci) % 3 == 0:  # and from row to row as well
                                p[by, bx, 7] = 0
                                p[by, bx, 56] = int(rng.choice([-1000, 1000]))
                planes.append(fit(p, q[comps[ci][3]]))
            return dict(width=w, height=h, comps=comps, qtabs=q, planes=planes)
        return dict(name=name, family="saturation", make=make)

    out += [alternating("sat_420_alternating_chroma", "4:2:0", 70, 38), alternating("sat_422_alternating_chroma", "4:2:2", 71, 21),
            alternating("sat_440_alternating_chroma", "4:4:0", 21, 39)]
    return out


def outside_family():
    out = []

    def dense(name, sub, w, h, qv):
        def make():
            rng = rng_of(name)
            comps = jw.components(sub)
            _, _, shapes = jw.geometry(w, h, comps)
            planes = [rng.choice([-1023, 1023], s + (64,)).astype(np.int64) for s in shapes]
            return dict(width=w, height=h, comps=comps, qtabs={0: flat(qv), 1: flat(qv)}, planes=planes)
        return dict(name=name, family="outside", make=make, dense=True)

    def dc_only(name, sub, w, h):
        def make():
            comps = jw.components(sub)
            _, _, shapes = jw.geometry(w, h, comps)
            planes = []
            for s in shapes:
                p = np.zeros(s + (64,), dtype=np.int64)
                p[:, :, 0] = 100
                p[::2, 1::2, 0] = -100
                planes.append(p)
            return dict(width=w, height=h, comps=comps, qtabs={0: flat(255), 1: flat(255)}, planes=planes)
        return dict(name=name, family="outside", make=make, dense=False)

    out += [dense("out_gray_dense_q255", "gray", 24, 16, 255), dense("out_420_dense_q255", "4:2:0", 32, 16, 255), dense("out_444_dense_q40", "4:4:4", 16, 8, 40),
            dc_only("out_gray_dc100_q255", "gray", 24, 16), dc_only("out_444_dc100_q255", "4:4:4", 16, 16)]
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = colour_rule() + tables_family() + symbols_family() + saturation_family() + outside_family()
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def build(case):
    """-> (the file's bytes, the longest code used, the writer's arguments -- its coefficient planes among them, and under
    "per_table" the longest code used of every table)"""
    args = case["make"]()
    per_table = {}
    blob, longest = jw.write(report=per_table, **args)
    args["per_table"] = per_table
    return blob, longest, args


def coefficients_sha256(args):
    return hashlib.sha256(b"".join(np.ascontiguousarray(p, dtype="<i2").tobytes() for p in args["planes"])).hexdigest()


def measures(args):
    """-> [max |coef * q|, max |pass-1 output|, max |final output|] over the file"""
    m = [0, 0, 0]
    for p, c in zip(args["planes"], args["comps"]):
        for k, v in enumerate(jw.idct_domain(p, args["qtabs"][c[3]])):
            m[k] = max(m[k], int(v.max()))
    return m


# ---------------------------------------------------------------- files made at test time (compared with the oracle: no Pillow needed)
TINY_W, TINY_H = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 33), (1, 2, 3, 4, 5, 8, 9, 16, 17)


def tiny_files():
    """-> [(sampling, w, h, bytes)]: the 297 tiny sizes of 4:2:0, 4:2:2 and 4:4:0 with textured chroma -- dsw <= 2 and dsh == 1
    among them, where the upsamplers change form"""
    out = []
    for sub in ("4:2:0", "4:2:2", "4:4:0"):
        comps = jw.components(sub)
        for w in TINY_W:
            for h in TINY_H:
                rng = rng_of("tiny_%s_%d_%d" % (sub, w, h))
                _, _, shapes = jw.geometry(w, h, comps)
                planes = [textured(rng, s, dc=120, nac=8, ac=60, reach=30) for s in shapes]
                out.append((sub, w, h, jw.write(w, h, comps, {0: flat(8), 1: flat(9)}, planes)[0]))
    return out


CHROMA_GRID = np.concatenate([np.arange(0, 254, 2), [255]])          # 128 values on a stride of 2, 0 and 255 among them


def colour_sweep(adobe0):
    """1024 x 1024, 4:4:4, DC-only blocks at q = 8: every sample of a block is exactly dc + 128.  Cb along x and Cr along y
    over CHROMA_GRID, Y through all of 0..255.  -> (bytes, the (128, 128, 3) samples per block in component order)"""
    comps = jw.components("4:4:4")
    by, bx = np.mgrid[0:128, 0:128]
    samples = np.stack([(bx * 37 + by * 101) % 256, CHROMA_GRID[bx], CHROMA_GRID[by]], axis=-1)
    samples[0, 0, 0], samples[127, 127, 0], samples[0, 127, 0], samples[127, 0, 0] = 255, 0, 0, 255     # the extremes meet
    planes = []
    for ci in range(3):
        p = np.zeros((128, 128, 64), dtype=np.int64)
        p[:, :, 0] = samples[:, :, ci] - 128
        planes.append(p)
    kw = dict(jfif=False, adobe=0) if adobe0 else {}
    return jw.write(1024, 1024, comps, {0: flat(8), 1: flat(8)}, planes, **kw)[0], samples


def hard_stream(sub, dri):
    """320 x 240: 60 % all-zero blocks (two or three bits each: a 32-byte chunk begins about a hundred of them) mixed with
    dense blocks, ZRL runs in front of coefficient 63 and DC swings of category 11.  -> (bytes, the planes)"""
    rng = rng_of("hard_%s_%d" % (sub, dri))
    comps = jw.components(sub)
    _, _, shapes = jw.geometry(320, 240, comps)
    planes = []
    for s in shapes:
        p = np.zeros(s + (64,), dtype=np.int64)
        kind = rng.random(s)
        run = np.cumsum(rng.random(s[0] * s[1]) < 0.04).reshape(s) % 4 == 0   # a quarter in long stretches of nothing but zero blocks
        for by in range(s[0]):
            for bx in range(s[1]):
                k = kind[by, bx]
                if k < 0.467 or run[by, bx]:           # 0.25 + 0.75 * 0.467 = 0.6
                    continue
                if k < 0.6:
                    p[by, bx] = rng.integers(-255, 256, 64)
                elif k < 0.75:
                    p[by, bx, 0] = int(rng.choice([-1023, 1023]))
                    p[by, bx, 63] = int(rng.integers(1, 4))
                elif k < 0.9:
                    p[by, bx, 0] = int(rng.choice([-1023, 1023]))
                else:
                    p[by, bx, rng.integers(1, 64, 3)] = rng.integers(-1023, 1024, 3)
        planes.append(p)
    return jw.write(320, 240, comps, {0: flat(1), 1: flat(1)}, planes, dri=dri)[0], planes


# ---------------------------------------------------------------- the domain rule, measured
def domain_study(pillow_bgr, orc):
    """Random gray blocks on both sides of the rule, 45 to a file: where do Pillow's libjpeg-turbo and the oracle's 32-bit
    IDCT with saturation disagree?  -> the figures DESIGN 4b and oracle/orc_jpeg.c quote"""
    rng = np.random.Generator(np.random.PCG64(20260))
    st = dict(in_domain_blocks=0, in_domain_disagreements=0, in_domain_peak_output=0, outside_blocks=0, outside_disagreements=0,
              smallest_disagreeing_pass1_peak=None, smallest_disagreeing_dequantised_peak=None)
    comps = jw.components("gray")
    for qv in (1, 2, 7, 16, 50, 255):
        for density in (0.05, 0.15, 0.4, 1.0):
            for reach in (1500, 6000, 16383, 30000, 120000):     # the largest |coef * q| drawn
                amp = max(1, min(1023, reach // qv))
                p = rng.integers(-amp, amp + 1, (5, 9, 64)) * (rng.random((5, 9, 64)) < density)
                blob, _ = jw.write(72, 40, comps, {0: flat(qv)}, [p])
                got, want = orc.jpeg_decode(blob)[1][:, :, 0], pillow_bgr(blob)
                a, b, f = jw.idct_domain(p, flat(qv))
                for by in range(5):
                    for bx in range(9):
                        same = np.array_equal(got[8 * by:8 * by + 8, 8 * bx:8 * bx + 8], want[8 * by:8 * by + 8, 8 * bx:8 * bx + 8])
                        if a[by, bx] <= jw.DOMAIN_LIMIT and b[by, bx] <= jw.DOMAIN_LIMIT:
                            st["in_domain_blocks"] += 1
                            st["in_domain_disagreements"] += not same
                            st["in_domain_peak_output"] = max(st["in_domain_peak_output"], int(f[by, bx]))
                        else:
                            st["outside_blocks"] += 1
                            if not same:
                                st["outside_disagreements"] += 1
                                for key, v in (("smallest_disagreeing_pass1_peak", b), ("smallest_disagreeing_dequantised_peak", a)):
                                    st[key] = int(v[by, bx]) if st[key] is None else min(st[key], int(v[by, bx]))
    assert st["in_domain_disagreements"] == 0, st
    return st


# ---------------------------------------------------------------- the folder
def npz_bytes(arrays):
    """np.savez_compressed without the clock in it"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            one = io.BytesIO()
            np.lib.format.write_array(one, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, one.getvalue(), compresslevel=9)
    return buf.getvalue()


def generate():
    """-> {file name: bytes} of the whole folder"""
    from PIL import Image, features
    import oracle_lib as orc

    def pillow_bgr(blob):
        a = np.asarray(Image.open(io.BytesIO(blob)))
        return a if a.ndim == 2 else a[:, :, ::-1]

    files, expected, entries = {}, {}, []
    covered = set()
    for case in cases():
        blob, longest, args = build(case)
        m = measures(args)
        inside = m[0] <= jw.DOMAIN_LIMIT and m[1] <= jw.DOMAIN_LIMIT
        assert inside == (case["family"] != "outside"), (case["name"], m)
        assert args["width"] <= 72 and args["height"] <= 40 and len(blob) < 8192, case["name"]
        want = pillow_bgr(blob)
        rc, got = orc.jpeg_decode(blob)
        assert rc == 0, (case["name"], rc)
        if inside:
            assert np.array_equal(got.reshape(want.shape), want), "the domain rule is wrong: %s %r" % (case["name"], m)
            expected[case["name"]] = want.reshape(got.shape)
        e = dict(name=case["name"], family=case["family"], in_domain=inside, shape=list(got.shape), bytes=len(blob), longest_code=longest,
                 coefficients_sha256=coefficients_sha256(args), max_dequantised=m[0], max_pass1=m[1], max_output=m[2],
                 verdict=case.get("verdict", 0),
                 options=dict(sof=args.get("sof", 0xC0), pq=str(args.get("pq", 0)), dri=args.get("dri", 0), fill=args.get("fill", 0),
                              ids=[c[0] for c in args["comps"]], sampling=[[c[1], c[2]] for c in args["comps"]], tq=[c[3] for c in args["comps"]],
                              tables=args.get("tables"), jfif=args.get("jfif", True), adobe=args.get("adobe"),
                              one_dht=args.get("one_dht", False), one_dqt=args.get("one_dqt", False), skew=bool(args.get("skew"))))
        if "ycc" in case:
            e["ycc"] = case["ycc"]
        entries.append(e)
        files[case["name"] + ".jpg"] = blob
        if case.get("kind") == "cat":
            n = case["first"]
            for p in args["planes"]:
                for _ in range(p.shape[0] * p.shape[1]):
                    covered.add((n % 63 + 1, SINGLE[n % 5]))
                    n += 1
        if case.get("kind") == "long":                   # 16-bit codes are USED in every DC and every AC table of the file
            e["longest_code_per_table"] = {"%s%d" % k: v for k, v in sorted(args["per_table"].items())}
            assert set(args["per_table"]) == set(args["skew"]) and all(v == 16 for v in args["per_table"].values()), (case["name"], args["per_table"])
    assert len(covered) == 63 * 5                        # every AC value at every zig-zag position, across the family
    sat = [e for e in entries if e["family"] == "saturation"]
    assert max(e["max_output"] for e in sat) > 2000 and all(e["max_output"] > 512 for e in sat)
    files["expected.npz"] = npz_bytes(expected)
    manifest = dict(pillow=__import__("PIL").__version__, libjpeg_turbo=features.version("libjpeg_turbo"), numpy=np.__version__,
                    domain_limit=jw.DOMAIN_LIMIT, domain_study=domain_study(pillow_bgr, orc), cases=entries)
    head = ["%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(manifest.items()) if k != "cases"]
    files["manifest.json"] = ("{\n" + ",\n".join(head) + ',\n"cases": [\n' + ",\n".join(json.dumps(e, sort_keys=True) for e in entries) + "\n]\n}\n").encode()
    return files


def main():
    files = generate()
    if "--check" in sys.argv:
        have = {n for n in os.listdir(OUT) if n.endswith((".jpg", ".npz", ".json"))}
        assert have == set(files), sorted(have ^ set(files))
        for n, b in files.items():
            with open(os.path.join(OUT, n), "rb") as f:
                assert f.read() == b, n
        print("jpeg_hand: %d files reproduced byte for byte" % len(files))
        return
    os.makedirs(OUT, exist_ok=True)
    for n, b in files.items():
        with open(os.path.join(OUT, n), "wb") as f:
            f.write(b)
    m = json.loads(files["manifest.json"])
    print("jpeg_hand: %d files, %d bytes; study %r" % (len(files), sum(len(b) for b in files.values()), m["domain_study"]))


if __name__ == "__main__":
    main()
