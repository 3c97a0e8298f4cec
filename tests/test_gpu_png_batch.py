"""impgpu_batch_decode_png: many PNG files in one call -- every file's code and pixels exactly what impgpu_image_decode_png
gives it alone (and what Pillow gives), refused and damaged files beside good ones, the launch count, the split of a batch
into staging groups, the frames entering the operator chain, and four threads decoding batches at once."""
import io
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
from PIL import Image

import oracle_lib as O
from conftest import ROOT
from png_writer import write_png

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "png")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))["files"]
EXPECTED = np.load(os.path.join(GOLD, "expected_pixels.npz"))


def reference_order(arr):
    if arr.ndim == 2:
        return arr[:, :, None]
    if arr.shape[2] == 1:
        return arr
    return arr[:, :, [2, 1, 0] + ([3] if arr.shape[2] == 4 else [])]


def pixels(im):
    a = im.numpy()
    return a if a.ndim == 3 else a[:, :, None]


def pillow(blob):
    return reference_order(np.asarray(Image.open(io.BytesIO(blob))))


def png_of(arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(b, "PNG", **kw)
    return b.getvalue()


def single(imp, blob):
    rc, im = imp.Image.decode_png(blob)
    return rc, (pixels(im) if rc == 0 else None)


@pytest.mark.parametrize("order", ["manifest", "shuffled"])
def test_golden_files_in_one_call(gpu, order):
    """every fixture -- good, refused (palette, gray + alpha, 16-bit, interlaced) and damaged -- in ONE call"""
    imp = gpu
    names = sorted(MANIFEST)
    if order == "shuffled":
        names = [names[i] for i in np.random.default_rng(11).permutation(len(names))]
    blobs = [open(os.path.join(GOLD, n), "rb").read() for n in names]
    res, launches = imp.batch_decode_png(blobs)
    assert len(res) == len(names)
    for name, (rc, im) in zip(names, res):
        assert rc == MANIFEST[name]["code"], (name, MANIFEST[name]["note"])
        if rc == 0:
            assert np.array_equal(pixels(im), EXPECTED[name]), name
        else:
            assert im is None
    assert launches <= len({EXPECTED[n].shape[2] for n in names if MANIFEST[n]["code"] == 0})


def _random_files(rng, n):
    """files of tests/png_writer.py: 1 / 3 / 4 channels, every filter type, levels 0 / 1 / 6 / 9, several IDAT chunks,
    sizes from 1 x 1 up to 4096 x 70 and 61 x 1500"""
    fixed = [(1, 1), (4096, 70), (61, 1500), (1, 300), (300, 1), (4095, 3), (65, 129)]
    out = []
    for k in range(n):
        c = int(rng.choice([1, 3, 4]))
        if k < len(fixed):
            w, h = fixed[k]
        else:
            w = int(rng.choice([int(rng.integers(1, 12)), int(rng.integers(1, 300)), int(rng.integers(1, 1500))]))
            h = int(rng.integers(1, 200)) if w < 400 else int(rng.integers(1, 90))
        if k % 3 == 0:
            arr = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            arr = np.stack([(xx * (k % 7 + 1) + yy * (ch + 2) + rng.integers(0, 5, size=(h, w))) % 256 for ch in range(c)], axis=2).astype(np.uint8)
        kinds = [int(v) for v in rng.integers(0, 5, size=h)]
        blob = write_png(arr[:, :, 0] if c == 1 else arr, kinds, {1: 0, 3: 2, 4: 6}[c], pieces=int(rng.integers(1, 5)),
                         level=int([0, 1, 6, 9][k % 4]))
        out.append((blob, reference_order(arr if c > 1 else arr[:, :, 0])))
    return out


def test_random_files_batch_equals_single_equals_pillow(gpu):
    imp = gpu
    files = _random_files(np.random.default_rng(20261015), 64)
    res, launches = imp.batch_decode_png([b for b, _ in files])
    assert launches <= 3
    for k, ((blob, want), (rc, im)) in enumerate(zip(files, res)):
        assert np.array_equal(pillow(blob), want), "the test's own encoder wrote a file Pillow reads differently"
        src, one = single(imp, blob)
        assert rc == 0 and src == 0, (k, rc, src)
        got = pixels(im)
        assert np.array_equal(got, one), k
        assert np.array_equal(got, want), k


def test_full_batch_of_256(gpu):
    imp = gpu
    rng = np.random.default_rng(256)
    blobs = []
    for k in range(256):
        c = [1, 3, 4][k % 3]
        h, w = int(rng.integers(1, 120)), int(rng.integers(1, 160))
        blobs.append(png_of(rng.integers(0, 256, size=(h, w, c), dtype=np.uint8) // int(rng.integers(1, 30)), compress_level=k % 10))
    res, launches = imp.batch_decode_png(blobs)
    assert launches == 3
    for blob, (rc, im) in zip(blobs, res):
        assert rc == 0 and np.array_equal(pixels(im), pillow(blob))
    with pytest.raises(imp.ImpError) as e:
        imp.batch_decode_png(blobs + blobs[:1])
    assert e.value.code == imp.IMP_ERROR_INVALID_ARGS


def test_size_limits_inside_a_batch(gpu):
    """a file 4097 wide and one 16385 high are refused; their neighbours decode as they would alone"""
    imp = gpu
    from ngx_http_imgproc_amd.workloads import photo_like

    good = [png_of(photo_like(40 + 9 * k, 50 + 13 * k, 3)) for k in range(3)]
    wide = png_of(np.zeros((4, 4097, 3), np.uint8))
    tall = png_of(np.zeros((16385, 2, 1), np.uint8))
    edge = png_of(np.full((3, 4096, 4), 7, np.uint8))
    blobs = [good[0], wide, good[1], tall, edge, good[2], b"not a png", b""]
    res, _ = imp.batch_decode_png(blobs)
    assert [rc for rc, _ in res] == [0, O.UNSUPPORTED, 0, O.UNSUPPORTED, 0, 0, O.UNSUPPORTED, O.UNSUPPORTED]
    for blob, (rc, im) in zip(blobs, res):
        assert rc == single(imp, blob)[0]
        if rc == 0:
            assert np.array_equal(pixels(im), pillow(blob))


def test_launches_one_per_channel_count(gpu):
    """the call launches k_png_unfilter_batch once per channel count present and nothing else (no copy or fill kernels)"""
    imp = gpu
    rng = np.random.default_rng(3)
    by_c = {c: [png_of(rng.integers(0, 256, size=(30, 20 + i, c), dtype=np.uint8)) for i in range(5)] for c in (1, 3, 4)}
    damaged = bytearray(by_c[3][0])
    damaged[45] ^= 0xFF                                     # inside the IDAT chunk: its CRC no longer matches
    for cs, want in (((3,), 1), ((1, 4), 2), ((1, 3, 4), 3)):
        blobs = [b for c in cs for b in by_c[c]]
        res, launches = imp.batch_decode_png(blobs + [bytes(damaged)])
        assert launches == want, cs
        assert all(rc == 0 for rc, _ in res[:-1]) and res[-1][0] == O.DECODE_FAILED
    res, launches = imp.batch_decode_png([bytes(damaged), b"\x89PNG"])
    assert launches == 0 and [rc for rc, _ in res] == [O.DECODE_FAILED, O.UNSUPPORTED]
    res, launches = imp.batch_decode_png([])
    assert res == [] and launches == 0


_CHILD = r"""
import io, json, sys
import numpy as np
from PIL import Image
sys.path.insert(0, sys.argv[1])
import ngx_http_imgproc_amd as imp
from ngx_http_imgproc_amd.workloads import photo_like
imp.env_start(0)
blobs = []
for k in range(20):
    b = io.BytesIO()
    Image.fromarray(photo_like(480, 640, 100 + k)).save(b, "PNG", compress_level=1)
    blobs.append(b.getvalue())
res, launches = imp.batch_decode_png(blobs)
ok = 0
for blob, (rc, im) in zip(blobs, res):
    want = np.asarray(Image.open(io.BytesIO(blob)))[:, :, ::-1]
    ok += int(rc == 0 and np.array_equal(im.numpy(), want))
del res, im
imp.env_destroy()
print(json.dumps({"ok": ok, "launches": launches}))
"""


def test_staging_cap_splits_the_batch(gpu):
    """IMPGPU_STAGE_CAP_MB=16 (a fresh process: the cap is read once): twenty 640 x 480 RGB files (0.92 MB of scanlines each)
    go in two groups of their own upload and launch, with the same pixels"""
    env = dict(os.environ, IMPGPU_STAGE_CAP_MB="16")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r == {"ok": 20, "launches": 2}, r


def test_batch_frames_enter_the_operator_chain(gpu):
    """batch-decoded frames through impgpu_batch_run_ops (resize=224,0) equal the oracle's resize of Pillow's pixels"""
    imp = gpu
    from ngx_http_imgproc_amd.workloads import photo_like

    blobs = [png_of(photo_like(300 + 20 * k, 400 - 10 * k, 3)) for k in range(6)]
    blobs.append(png_of(np.dstack([photo_like(260, 330, 3), np.full((260, 330, 1), 200, np.uint8)])))
    res, _ = imp.batch_decode_png(blobs)
    assert all(rc == 0 for rc, _ in res)
    ims = [im for _, im in res]
    cfg = imp.Config()
    out, _ = imp.batch_run_ops(ims, [cfg] * len(ims), [dict(resize="224,0")] * len(ims))
    for blob, im, (rc, step) in zip(blobs, ims, out):
        orc, want = O.resize(np.ascontiguousarray(pillow(blob)), "224,0")
        assert rc == 0 and orc == 0 and np.array_equal(pixels(im), want)


def test_four_threads_decode_their_own_batches(gpu):
    imp = gpu
    from ngx_http_imgproc_amd.workloads import photo_like

    work = []
    for t in range(4):
        blobs = [png_of(photo_like(120 + 17 * k + t, 160 + 11 * k, 3)[:, :, :[1, 3, 3, 3][k % 4]].copy(), compress_level=(k + t) % 10)
                 for k in range(12)]
        work.append(blobs)
    errors = []
    start = threading.Barrier(4)

    def one(t):
        try:
            start.wait()
            for _ in range(3):
                res, _ = imp.batch_decode_png(work[t])
                for blob, (rc, im) in zip(work[t], res):
                    if rc != 0 or not np.array_equal(pixels(im), pillow(blob)):
                        errors.append((t, rc))
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append((t, repr(e)))

    ts = [threading.Thread(target=one, args=(t,)) for t in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[:5]
