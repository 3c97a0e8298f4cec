"""The baseline JPEG front on the device -- k_jpeg_walks, _mend, _select, _write, _dcfix, k_jpeg_entropy_small and
k_jpeg_pixels<HS,VS,NC> -- on hand-written files (jpeg_writer.py, tests/golden/jpeg_hand/): untransformed RGB, three
quantisation tables, 16-bit tables, every selector mix, DC differences of category 11, AC category 10, 15- and 16-bit
codes, ZRL runs, blocks without EOB, one-MCU restart intervals, saturation far outside 0..255 and streams of all-zero
blocks.  The committed files are compared with PILLOW's pixels; the files made at test time with the oracle, which is
the same 32-bit arithmetic with saturation as the kernel (no Pillow needed here).
"""
import json
import os

import numpy as np
import pytest

import make_jpeg_hand as gen
import oracle_lib as orc
from test_gpu_jpeg import MODES, decode, huff  # noqa: F401  (huff: the fixture that runs a test in every entropy mode)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_hand")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
EXPECTED = np.load(os.path.join(GOLD, "expected.npz"))
ENTRY = {e["name"]: e for e in MANIFEST["cases"]}
NAMES = [e["name"] for e in MANIFEST["cases"]]
INSIDE = [n for n in NAMES if ENTRY[n]["in_domain"]]
OUTSIDE = [n for n in NAMES if not ENTRY[n]["in_domain"]]
_cache = {}


@pytest.fixture(autouse=True)
def _device_entropy_unless_a_test_says_otherwise(monkeypatch):
    """It is the DEVICE's entropy stage these files are here for: unset, a lone small file's runs on the calling thread."""
    monkeypatch.setenv("IMPGPU_JPEG_HUFF", "device")


def committed(name):
    with open(os.path.join(GOLD, name + ".jpg"), "rb") as f:
        return f.read()


def once(key, make):
    """the files the Python writer takes a while over are built once per module"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def timeouts(gpu):
    return gpu.jpeg_counters()[2]


def on_device(gpu):
    """-> (files whose entropy stage ran on the device, files kept on the calling thread for their long blocks)"""
    c = gpu.jpeg_counters()
    return c[0], c[3]


def batch(gpu, blobs):
    """-> [(code, pixels or None)]"""
    out = []
    for code, im in gpu.batch_decode_jpeg(blobs):
        out.append((code, None if im is None else im.numpy()))
        if im is not None:
            im.release()
    return out


@pytest.mark.parametrize("name", INSIDE)
def test_lone_files_decode_to_pillows_pixels(gpu, huff, name):
    e = ENTRY[name]
    ran, kept = on_device(gpu)
    rc, got = decode(gpu, committed(name))
    assert rc == e["verdict"]
    if huff == "device":                                 # no quiet way round the device's entropy stage
        assert on_device(gpu) == (ran + (rc == 0), kept)
    if rc == 0:
        assert list(got.shape) == e["shape"]
        assert np.array_equal(got, EXPECTED[name]), (name, int(np.abs(got.astype(int) - EXPECTED[name]).max()))
    else:
        assert rc == gpu.IMP_ERROR_UNSUPPORTED           # three different Huffman tables: left to the caller's host decoder


def test_one_batch_of_every_file(gpu, huff):
    """Mixed samplings in one call: a pixel launch per class, tile maps over frames of 1 to 72 pixels."""
    blobs = [committed(n) for n in NAMES]
    before = timeouts(gpu)
    ran, kept = on_device(gpu)
    res = batch(gpu, blobs)
    assert len(res) == len(NAMES)
    if huff == "device":
        assert on_device(gpu) == (ran + sum(e["verdict"] == 0 for e in MANIFEST["cases"]), kept)
    for name, blob, (code, got) in zip(NAMES, blobs, res):
        e = ENTRY[name]
        assert code == e["verdict"], name
        lone_rc, lone = decode(gpu, blob)
        assert lone_rc == code
        if code:
            assert got is None
            continue
        assert list(got.shape) == e["shape"] and np.array_equal(got, lone), name
        if e["in_domain"]:
            assert np.array_equal(got, EXPECTED[name]), name
    assert timeouts(gpu) == before


@pytest.mark.parametrize("name", OUTSIDE)
def test_out_of_domain_files_are_the_32_bit_restatement_in_every_mode(gpu, monkeypatch, name):
    """No expected pixels are committed for these: libjpeg-turbo's SIMD IDCT, plain-C libjpeg and 32-bit arithmetic with
    saturation give three answers.  The product's is the third, like the oracle's, wherever the entropy stage ran."""
    blob = committed(name)
    got = {}
    for mode in MODES:
        if mode == "auto":
            monkeypatch.delenv("IMPGPU_JPEG_HUFF", raising=False)
        else:
            monkeypatch.setenv("IMPGPU_JPEG_HUFF", mode)
        rc, got[mode] = decode(gpu, blob)
        assert rc == 0 and list(got[mode].shape) == ENTRY[name]["shape"]
    assert np.array_equal(got["device"], got["host"]) and np.array_equal(got["device"], got["auto"])
    if ENTRY[name]["max_pass1"] * 2048 >= 2 ** 31:
        # the oracle's `int` arithmetic overflows on this file (undefined in C): already the pass-1 value before its descale by
        # 11 bits does not fit 32 bits (the three dense files; not the DC-only ones).  Only the cross-mode comparison is kept.
        assert "dense" in name
        return
    assert "dc100" in name
    rc, want = orc.jpeg_decode(blob)
    assert rc == 0 and np.array_equal(got["device"], want)


def test_tiny_sizes(gpu, huff):
    """297 sizes from 1 x 1 of the three subsampled classes, textured chroma: the replicating upsamplers (dsw <= 2), one
    chroma row (dsh == 1), the first and last columns' clamps -- in one batched call, and a dozen lone."""
    files = once("tiny", gen.tiny_files)
    assert len(files) == 297
    wants = once("tiny_want", lambda: [orc.jpeg_decode(f[3])[1] for f in files])
    res = batch(gpu, [f[3] for f in files])
    for (sub, w, h, _), want, (code, got) in zip(files, wants, res):
        assert code == 0 and got.shape == (h, w, 3), (sub, w, h)
        assert np.array_equal(got, want), (sub, w, h)
    for i in range(5, 297, 25):
        rc, got = decode(gpu, files[i][3])
        assert rc == 0 and np.array_equal(got, wants[i]), files[i][:3]


@pytest.mark.parametrize("adobe0", [False, True], ids=["ycbcr", "adobe0-rgb"])
def test_colour_sweep(gpu, adobe0):
    """Every (Cb, Cr) of a stride-2 grid with 0 and 255, Y through 0..255: the samples are exactly dc + 128, so the colour
    stage alone is under test -- its 16-bit fixed point and its saturation, or the untransformed R,G,B -> B,G,R."""
    blob, samples = once(("sweep", adobe0), lambda: gen.colour_sweep(adobe0))
    rc, got = decode(gpu, blob)
    assert rc == 0 and got.shape == (1024, 1024, 3)
    rc, want = once(("sweep_want", adobe0), lambda: orc.jpeg_decode(blob))
    assert rc == 0
    blocks = got[::8, ::8]
    assert np.array_equal(got, np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1))
    if adobe0:
        assert np.array_equal(blocks, samples[:, :, ::-1])
    else:                                               # jdcolor.c's tables, restated in numpy
        y, cb, cr = (samples[:, :, k].astype(np.int64) for k in range(3))
        r = y + ((91881 * (cr - 128) + 32768) >> 16)
        g = y + ((-22554 * (cb - 128) - 46802 * (cr - 128) + 32768) >> 16)
        b = y + ((116130 * (cb - 128) + 32768) >> 16)
        assert np.array_equal(blocks, np.clip(np.stack([b, g, r], axis=-1), 0, 255))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dri", [0, 5])
@pytest.mark.parametrize("sub", ["4:2:0", "4:4:4"])
def test_hard_stream(gpu, sub, dri):
    """60 % all-zero blocks among dense, ZRL and category-11 blocks, long enough for several k_jpeg_select workgroups: lone
    (the fused kernel), in a batch of over 192 KB (the five-kernel path); the 4:4:4 file without restarts once more in a
    batch of over 4 MB (256-byte chunks).  No wait between workgroups times out."""
    blob, _ = once(("hard", sub, dri), lambda: gen.hard_stream(sub, dri))
    assert len(blob) > 256 * 32 * 2
    rc, want = orc.jpeg_decode(blob)
    assert rc == 0
    before = timeouts(gpu)
    ran, kept = on_device(gpu)
    rc, got = decode(gpu, blob)
    assert rc == 0 and np.array_equal(got, want)
    assert timeouts(gpu) == before and on_device(gpu) == (ran + 1, kept)
    sizes = [(192 << 10) // len(blob) + 2]
    if sub == "4:4:4" and dri == 0:
        sizes.append((4 << 20) // len(blob) + 2)
    for copies in sizes:
        assert copies * len(blob) > (192 << 10) and copies <= 256
        ran, kept = on_device(gpu)
        res = batch(gpu, [blob] * copies)
        assert len(res) == copies and on_device(gpu) == (ran + copies, kept)
        for code, got in res:
            assert code == 0 and np.array_equal(got, want)
        assert timeouts(gpu) == before
