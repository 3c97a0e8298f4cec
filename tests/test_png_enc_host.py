"""The PNG encoder's deflate on the host (no device): impgpu_png_deflate runs the kernels' own symbol / tree / bit code
(csrc/imp_png_deflate.h) and must give zlib 1.2.11's Z_RLE stream byte for byte; the Python model of the whole file is
pinned to the libpng fixtures, and to libpng itself where it can be loaded."""
import json
import os
import zlib

import numpy as np
import pytest

import ngx_http_imgproc_amd as imp
import png_enc_model as model

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "png_enc")


def zlib_rle(data):
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return co.compress(data) + co.flush()


def check(data):
    rc, got = imp.png_deflate(data)
    assert rc == 0
    want = model.zlib_stream(data)               # zlib's stream with libpng's header rule
    assert got == want, "stream of %d bytes differs" % len(data)
    assert got[2:] == zlib_rle(data)[2:]


def fib_stream(nsym, seed):
    """Literal frequencies in a Fibonacci spread (deep trees: gen_bitlen's 15-bit repair), no runs of 4."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    syms = np.concatenate([np.full(f, v, np.uint8) for v, f in zip(range(0, 220, 10), fib)])
    rng = np.random.default_rng(seed)
    rng.shuffle(syms)
    syms = syms[:nsym]
    # break runs: equal neighbours become matches, not literals
    for i in range(1, len(syms)):
        if syms[i] == syms[i - 1]:
            syms[i] = (int(syms[i]) + 5) % 256
    return syms.tobytes()


def test_special_streams():
    check(b"")
    check(b"\x00")
    # a run-free stream of exactly 16383 k symbols: the final block is an empty fixed block (03 00)
    for k in (1, 2, 3):
        data = (np.arange(16383 * k) % 251).astype(np.uint8).tobytes()
        rc, got = imp.png_deflate(data)
        assert rc == 0 and got == model.zlib_stream(data)
    check(fib_stream(17000, 1))
    check(fib_stream(40000, 2))
    for L in (1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 516, 517, 518, 100000):
        check(b"a" * L)
        check(b"xy" + b"a" * L + b"z")
    check(bytes(4_500_000))                      # all matches: blocks of 16383 symbols over 4 MB each
    check(np.random.default_rng(3).integers(0, 256, 300_000, dtype=np.uint8).tobytes())   # stored blocks


def test_random_streams():
    rng = np.random.default_rng(0x9E37)
    for i in range(2000):
        n = int(rng.integers(1, 3000 if i < 1500 else 70000))
        kind = i % 5
        if kind == 0:
            d = rng.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1:
            d = rng.integers(0, 3, n, dtype=np.uint8)
        elif kind == 2:
            d = np.repeat(rng.integers(0, 256, n // 4 + 1, dtype=np.uint8), rng.integers(1, 300, n // 4 + 1))[:n]
        elif kind == 3:
            d = (rng.geometric(0.2, n) % 256).astype(np.uint8)
        else:
            d = np.frombuffer(model.filter_rows(model.make_frame("smooth", 3, max(1, n // 9), 3, i)), np.uint8)
        check(d.tobytes())


def test_capacity():
    data = bytes(range(256)) * 10
    n = imp.ops.C.c_size_t()
    buf = np.empty(8, np.uint8)
    rc = imp.lib.impgpu_png_deflate(data, len(data), buf.ctypes.data, 8, imp.ops.C.byref(n))
    assert rc == imp.IMP_ERROR_MALLOC_FAILED and n.value > 8


def test_bound_and_refusals():
    assert imp.lib.impgpu_png_encode_bound(224, 224, 3) >= len(model.encode(model.make_frame("noise", 224, 224, 3)))
    assert imp.lib.impgpu_png_encode_bound(224, 224, 2) == 0
    assert imp.lib.impgpu_png_encode_bound(0, 5, 3) == 0
    # libpng's write limits (PNG_USER_WIDTH_MAX / HEIGHT_MAX): cvEncodeImage fails beyond them, so the device refuses them too
    assert imp.lib.impgpu_png_encode_bound(1_000_000, 1, 1) > 0 and imp.lib.impgpu_png_encode_bound(1, 1_000_000, 1) > 0
    assert imp.lib.impgpu_png_encode_bound(1_000_001, 1, 1) == 0 and imp.lib.impgpu_png_encode_bound(1, 1_000_001, 1) == 0


def fixtures():
    with open(os.path.join(GOLD, "manifest.json")) as fh:
        man = json.load(fh)
    files = np.load(os.path.join(GOLD, "cases.npz"))
    return man, files


def test_model_matches_fixtures():
    man, files = fixtures()
    assert man["libpng"].startswith("1.6.") and man["zlib"] == "1.2.11"
    for case in man["cases"]:
        frame = model.make_frame(case["kind"], case["h"], case["w"], case["c"], case["seed"])
        assert model.encode(frame) == files[case["key"]].tobytes(), case


def test_fixtures_hold_a_stream_of_whole_chunks():
    """A zlib stream of exactly k * 8192 bytes ends with a full IDAT chunk and no empty one after it."""
    man, files = fixtures()
    whole = [c for c in man["cases"] if c["bytes"] > 45 and (c["bytes"] - 45) % (8192 + 12) == 0]
    assert whole
    for case in whole:
        blob = files[case["key"]].tobytes()
        assert blob[-12:-8] == b"\x00\x00\x00\x00" and blob[-20:-12] != b"\x00\x00\x00\x00IDAT"


def test_deflate_matches_fixture_streams():
    """The host run of the device code over each fixture's filtered rows gives the fixture's IDAT payload."""
    man, files = fixtures()
    for case in man["cases"]:
        if case["h"] * case["w"] > 400_000:
            continue
        frame = model.make_frame(case["kind"], case["h"], case["w"], case["c"], case["seed"])
        blob = files[case["key"]].tobytes()
        z, at = b"", 33
        while blob[at + 4:at + 8] == b"IDAT":
            n = int.from_bytes(blob[at:at + 4], "big")
            z += blob[at + 8:at + 8 + n]
            at += 12 + n
        rc, got = imp.png_deflate(model.filter_rows(frame))
        assert rc == 0 and got == z, case


def test_model_matches_live_libpng():
    lib = model.load_libpng()
    if lib is None:
        pytest.skip("libpng16 is not loadable here")
    rng = np.random.default_rng(11)
    for i in range(40):
        h, w, c = int(rng.integers(1, 60)), int(rng.integers(1, 90)), int(rng.choice([1, 3, 4]))
        kind = ["smooth", "noise", "flat", "stripes5"][i % 4]
        frame = model.make_frame(kind, h, w, c, i)
        assert model.libpng_encode(lib, frame, 9) == model.encode(frame), (kind, h, w, c)
