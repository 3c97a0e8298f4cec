"""The hand-written baseline files of tests/golden/jpeg_hand/ on the host, no GPU: the marker parser, both entropy
decoders (the sequential one and the device's chunk-parallel scheme run lane by lane, imp_jpeg_core.h) and the oracle,
on what Pillow's encoder never writes (jpeg_writer.py).  The coefficients compared with are the ones the writer was
GIVEN -- regenerated from the seed and checked by the manifest's sha256 -- not ones read back through a decoder.
"""
import ctypes as C
import hashlib
import io
import json
import os

import numpy as np
import pytest

import jpeg_writer as jw
import make_jpeg_hand as gen
import oracle_lib as orc

import ngx_http_imgproc_amd as imp
from ngx_http_imgproc_amd._lib import lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_hand")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
EXPECTED = np.load(os.path.join(GOLD, "expected.npz"))
ENTRY = {e["name"]: e for e in MANIFEST["cases"]}
CASES = {c["name"]: c for c in gen.cases()}
NAMES = [e["name"] for e in MANIFEST["cases"]]
_built = {}


def committed(name):
    with open(os.path.join(GOLD, name + ".jpg"), "rb") as f:
        return f.read()


def built(name):
    """the file written again from its seed -> (bytes, longest code, the writer's arguments)"""
    if name not in _built:
        _built[name] = gen.build(CASES[name])
    return _built[name]


def written_coefficients(name):
    args = built(name)[2]
    assert gen.coefficients_sha256(args) == ENTRY[name]["coefficients_sha256"]
    return np.concatenate([np.asarray(p, dtype=np.int16).reshape(-1) for p in args["planes"]])


def product_coefficients(blob, how):
    out = np.zeros(200_000, dtype=np.int16)
    info = (C.c_int * 12)()
    rc = lib.impgpu_jpeg_coefficients(blob, len(blob), how, out.ctypes.data, out.size, info)
    return rc, out[: info[0]].copy() if rc == 0 else None, list(info)


def test_the_manifest_lists_the_generators_cases_and_the_folder():
    assert NAMES == [c["name"] for c in gen.cases()]
    on_disk = {n[:-4] for n in os.listdir(GOLD) if n.endswith(".jpg")}
    assert on_disk == set(NAMES)
    assert set(EXPECTED.files) == {n for n in NAMES if ENTRY[n]["in_domain"]}
    assert sum(not ENTRY[n]["in_domain"] for n in NAMES) in (4, 5, 6)
    st = MANIFEST["domain_study"]
    assert st["in_domain_disagreements"] == 0 and st["in_domain_blocks"] > 1000
    assert st["smallest_disagreeing_pass1_peak"] > jw.DOMAIN_LIMIT


@pytest.mark.parametrize("name", NAMES)
def test_written_again_from_the_seed_the_file_is_the_committed_one(name):
    blob, longest, args = built(name)
    e = ENTRY[name]
    assert blob == committed(name)
    assert longest == e["longest_code"]
    assert gen.measures(args) == [e["max_dequantised"], e["max_pass1"], e["max_output"]]
    assert (e["max_dequantised"] <= jw.DOMAIN_LIMIT and e["max_pass1"] <= jw.DOMAIN_LIMIT) == e["in_domain"]
    if "_long_" in name:                                 # codes of 16 bits are used, not only listed, in every DC and AC table
        per = {"%s%d" % k: v for k, v in args["per_table"].items()}
        assert per == e["longest_code_per_table"] and set(per.values()) == {16}
        assert set(per) == ({"dc0", "ac0"} if e["shape"][2] == 1 else {"dc0", "ac0", "dc1", "ac1"})


@pytest.mark.parametrize("how", [0, 1], ids=["sequential", "chunk-parallel"])
@pytest.mark.parametrize("name", NAMES)
def test_both_entropy_decoders_return_the_coefficients_the_writer_was_given(name, how):
    e = ENTRY[name]
    rc, got, info = product_coefficients(committed(name), how)
    assert rc == e["verdict"]
    if rc:
        return                                           # (three different Huffman tables: refused before the entropy stage)
    assert info[1] == 0                                  # the walks' status word: no bad code, no bad count
    want = written_coefficients(name)
    assert got.size == want.size and np.array_equal(got, want)


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_decodes_to_pillows_pixels_and_the_header_to_the_shape(name):
    e = ENTRY[name]
    blob = committed(name)
    rc, got = orc.jpeg_decode(blob)
    assert rc == 0 and list(got.shape) == e["shape"]
    if e["in_domain"]:
        assert np.array_equal(got, EXPECTED[name])
    h, w, c = e["shape"]
    assert imp.jpeg_info(blob) == (0, (w, h, c))
    assert lib.impgpu_jpeg_classify(blob, len(blob)) == 0
    for ci in range(c):                                  # and the oracle's own entropy decoder reads what was written
        rc, co = orc.jpeg_coefficients(blob, ci)
        assert rc == 0 and np.array_equal(co.reshape(-1), np.asarray(built(name)[2]["planes"][ci], dtype=np.int16).reshape(-1))


def test_pillow_opens_every_file():
    Image = pytest.importorskip("PIL.Image")
    for name in NAMES:
        im = Image.open(io.BytesIO(committed(name)))
        a = np.asarray(im)
        e = ENTRY[name]
        assert list(a.shape[:2]) == e["shape"][:2] and im.mode == ("L" if e["shape"][2] == 1 else "RGB")
        if e["in_domain"]:
            assert np.array_equal(a if a.ndim == 2 else a[:, :, ::-1], EXPECTED[name].reshape(a.shape))


def test_untransformed_files_read_as_r_g_b():
    """The colour rule's expected pixels are not the oracle's opinion: with a DC-only 4:4:4 file the samples are known
    in closed form, and an untransformed file's components arrive as R, G, B -> B, G, R."""
    rgb = [e for e in MANIFEST["cases"] if e["family"] == "colour" and not e["ycc"]]
    ycc = [e for e in MANIFEST["cases"] if e["family"] == "colour" and e["ycc"]]
    assert len(rgb) == 2 * (3 + 1) and len(ycc) == 36 - len(rgb)      # Adobe 0 without JFIF on any ids; 'R','G','B' with no marker
    comps = jw.components("4:4:4", (ord("R"), ord("G"), ord("B")))
    planes = [np.zeros((1, 1, 64), dtype=np.int64) for _ in range(3)]
    for p, dc in zip(planes, (-100, 20, 90)):
        p[0, 0, 0] = dc
    blob, _ = jw.write(8, 8, comps, {0: np.full(64, 8), 1: np.full(64, 8)}, planes, jfif=False)
    rc, got = orc.jpeg_decode(blob)
    assert rc == 0 and np.all(got == np.array([90 + 128, 20 + 128, -100 + 128], dtype=np.uint8))


def test_the_domain_helper():
    q = np.full(64, 13)
    for dc in (1, -7, 100, 315):
        blk = np.zeros(64, dtype=np.int64)
        blk[0] = dc
        a, b, f = jw.idct_domain(blk, q)
        assert (a, b) == (abs(dc) * 13, 4 * abs(dc) * 13)            # a DC-only block: pass 1 is the term times 2^PASS1_BITS
        assert f == (abs(dc * 13) + 4) // 8 or f == abs((dc * 13 + 4) >> 3)
    # against a float IDCT: the integer passes are within a sample of it
    rng = np.random.Generator(np.random.PCG64(3))
    coef = rng.integers(-200, 201, (50, 64))
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k == 0, np.sqrt(0.5), 1.0)[:, None] / 2
    ref = np.einsum("ux,vy,nuv->nxy", basis, basis, (coef * q).reshape(50, 8, 8).astype(np.float64))
    _, _, f = jw.idct_domain(coef, q)
    assert np.all(np.abs(f - np.abs(ref).reshape(50, 64).max(axis=1)) <= 1.0)
    assert jw.in_domain(coef // 8, q) and not jw.in_domain(np.full(64, 1023), np.full(64, 255))


def test_out_of_domain_files_decode_everywhere():
    for name in NAMES:
        if ENTRY[name]["in_domain"]:
            continue
        blob = committed(name)
        assert orc.jpeg_decode(blob)[0] == 0
        for how in (0, 1):
            assert product_coefficients(blob, how)[0] == 0


def test_the_deferred_files_verdict():
    deferred = [n for n in NAMES if ENTRY[n]["verdict"]]
    assert deferred == ["tab_444_three_huffman", "tab_420_three_dc_tables"]
    for name in deferred:
        blob = committed(name)
        assert ENTRY[name]["verdict"] == imp.IMP_ERROR_UNSUPPORTED
        for how in (0, 1):
            assert product_coefficients(blob, how)[0] == imp.IMP_ERROR_UNSUPPORTED
        assert imp.jpeg_info(blob)[0] == 0               # the header is fine: it is the entropy stage's two table slots that refuse
        assert hashlib.sha256(blob).hexdigest() == hashlib.sha256(built(name)[0]).hexdigest()
