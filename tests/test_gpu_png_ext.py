"""impgpu_image_decode_png_ex / impgpu_batch_decode_png_ex on the device: palette (depth 1/2/4/8), 1/2/4-bit gray and Adam7
files of every accepted kind decode to what libpng gives cvDecodeImage(blob, -1) -- Pillow's pixels, or the numpy model where a
palette index lies past the PLTE -- alone and in batches; today's kinds through _ex are the old calls' frames with the old
launch counts; launches do not grow with the file count; a decoded palette upload goes through the operator chain."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import png_ext_writer as W
from conftest import ROOT
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "png_ext")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
EXPECTED = np.load(os.path.join(GOLD, "expected_pixels.npz"))
OLD = os.path.join(ROOT, "tests", "golden", "png")


def pixels(im):
    a = im.numpy()
    return a if a.ndim == 3 else a[:, :, None]


def single(imp, blob, accept):
    rc, im = imp.Image.decode_png_ex(blob, accept)
    try:
        return rc, (pixels(im) if rc == 0 else None)
    finally:
        if im is not None:
            im.release()


def batch(imp, blobs, accept):
    res, launches = imp.batch_decode_png_ex(blobs, accept)
    out = []
    for rc, im in res:
        out.append((rc, pixels(im) if rc == 0 else None))
        if im is not None:
            im.release()
    return out, launches


def test_golden_files_single_and_batch(gpu):
    imp = gpu
    names = sorted(MANIFEST)
    blobs = [open(os.path.join(GOLD, n), "rb").read() for n in names]
    for name, blob in zip(names, blobs):
        rc, got = single(imp, blob, imp.PNG_ALL)
        assert rc == MANIFEST[name]["code"], name
        if rc == 0:
            assert np.array_equal(got, EXPECTED[name]), name
    res, launches = batch(imp, blobs, imp.PNG_ALL)
    for name, (rc, got) in zip(names, res):
        assert rc == MANIFEST[name]["code"], name
        if rc == 0:
            assert np.array_equal(got, EXPECTED[name]), name
    # unfilter: one launch per filter unit (1 / 3 / 4), place: one per channel count (1 / 3 / 4)
    assert launches <= 6
    # without the kind in the mask: refused as the old call refuses it
    for name, blob in zip(names, blobs):
        if MANIFEST[name]["code"] == 0:
            assert single(imp, blob, 0)[0] == imp.IMP_ERROR_UNSUPPORTED, name


def test_n_palette_decodes_and_n_interlaced_is_damaged(gpu):
    imp = gpu
    pal = open(os.path.join(OLD, "n_palette.png"), "rb").read()
    rc, got = single(imp, pal, imp.PNG_ALL)
    assert rc == 0 and got.shape == (12, 12, 3)
    assert np.array_equal(got, W.pillow(pal))
    assert single(imp, pal, imp.PNG_LOW_GRAY | imp.PNG_ADAM7)[0] == imp.IMP_ERROR_UNSUPPORTED
    il = open(os.path.join(OLD, "n_interlaced.png"), "rb").read()
    assert single(imp, il, imp.PNG_ALL)[0] == imp.IMP_ERROR_DECODE_FAILED
    assert single(imp, il, 0)[0] == imp.IMP_ERROR_UNSUPPORTED


KINDS = [(3, 1), (3, 2), (3, 4), (3, 8), (0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (6, 8)]


def _random_set(seed, n, max_w=300, max_h=120):
    """n random files of every accepted kind (today's 8-bit kinds interlaced only), with the expected pixels"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        colour, depth = KINDS[k % len(KINDS)]
        il = 1 if colour in (2, 6) or (colour == 0 and depth == 8) else int(rng.integers(0, 2))
        w, h = int(rng.integers(1, max_w + 1)), int(rng.integers(1, max_h + 1))
        oor = colour == 3 and rng.random() < 0.3
        n_pal = int(rng.integers(1, (1 << depth) + 1)) if colour == 3 else None
        blob, want = W.random_file(rng, colour, depth, il, w, h, n_pal=n_pal, out_of_range=oor)
        if not oor:
            assert np.array_equal(W.pillow(blob), want)          # the model is Pillow's decode wherever Pillow is libpng
        out.append((blob, want))
    return out


def test_seeded_random_files_single(gpu):
    imp = gpu
    for blob, want in _random_set(0x5EED, 60):
        rc, got = single(imp, blob, imp.PNG_ALL)
        assert rc == 0 and np.array_equal(got, want)


def test_wide_and_tiny_files(gpu):
    """1 x 1 up to 4096 wide, every kind, interlaced and not"""
    imp = gpu
    rng = np.random.default_rng(42)
    files = []
    for colour, depth in KINDS:
        for w, h in ((1, 1), (4096, 3), (4095, 9), (2, 17), (1025, 2)):
            for il in (0, 1):
                if il == 0 and (colour in (2, 6) or depth == 8 and colour == 0):
                    continue
                files.append(W.random_file(rng, colour, depth, il, w, h))
    res, _ = batch(imp, [b for b, _ in files], imp.PNG_ALL)
    for (blob, want), (rc, got) in zip(files, res):
        assert rc == 0 and np.array_equal(got, want), want.shape


def test_todays_kinds_through_ex_are_the_old_calls(gpu):
    imp = gpu
    names = sorted(os.path.basename(f) for f in os.listdir(OLD) if f.endswith(".png"))
    blobs = [open(os.path.join(OLD, n), "rb").read() for n in names]
    old, old_launches = imp.batch_decode_png(blobs)
    # (n_palette.png and n_interlaced.png are new kinds: under PNG_ALL they decode / fail, so they leave that batch)
    plain = [b for n, b in zip(names, blobs) if n not in ("n_palette.png", "n_interlaced.png")]
    _, plain_launches = imp.batch_decode_png(plain)
    res, all_launches = imp.batch_decode_png_ex(plain, imp.PNG_ALL)
    assert all_launches == plain_launches
    for _, im in res:
        if im is not None:
            im.release()
    for accept in (0, imp.PNG_LOW_GRAY):
        new, new_launches = imp.batch_decode_png_ex(blobs, accept)
        assert new_launches == old_launches
        for name, (rc0, im0), (rc1, im1) in zip(names, old, new):
            assert rc0 == rc1, (name, accept)
            if rc0 == 0:
                assert np.array_equal(im0.numpy(), im1.numpy()), name
                im1.release()
    for name, blob in zip(names, blobs):
        rc0, im0 = imp.Image.decode_png(blob)
        for accept in (0, imp.PNG_ALL):
            rc1, im1 = imp.Image.decode_png_ex(blob, accept)
            if rc0 == 0:
                assert rc1 == 0 and np.array_equal(im0.numpy(), im1.numpy()), name
                im1.release()
            elif accept == 0 or name not in ("n_palette.png", "n_interlaced.png"):
                assert rc1 == rc0, (name, accept)
        if im0 is not None:
            im0.release()
    for _, im in old:
        if im is not None:
            im.release()


def test_mixed_batch_of_256_equals_single_calls(gpu):
    imp = gpu
    files = _random_set(0xB17, 200, max_w=200, max_h=90)
    old = [open(os.path.join(OLD, n), "rb").read() for n in sorted(os.listdir(OLD)) if n.endswith(".png")]
    blobs = [b for b, _ in files] + old
    blobs = blobs[:256]
    order = np.random.default_rng(3).permutation(len(blobs))
    blobs = [blobs[i] for i in order]
    res, launches = batch(imp, blobs, imp.PNG_ALL)
    assert launches <= 6                                  # plain and item unfilter share 3 launches; place 3
    for blob, (rc, got) in zip(blobs, res):
        rc1, got1 = single(imp, blob, imp.PNG_ALL)
        assert rc == rc1
        if rc == 0:
            assert np.array_equal(got, got1)


def test_launches_do_not_grow_with_the_file_count(gpu):
    imp = gpu
    files = _random_set(0xC0C0, 128, max_w=64, max_h=40)
    counts = []
    for n in (len(KINDS), 64, 128):
        res, launches = batch(imp, [b for b, _ in files[:n]], imp.PNG_ALL)
        for (blob, want), (rc, got) in zip(files[:n], res):
            assert rc == 0 and np.array_equal(got, want)
        counts.append(launches)
    assert counts[0] == counts[1] == counts[2] <= 6, counts


def test_palette_upload_through_the_operator_chain(gpu):
    """decode_png_ex -> impgpu_run_ops (resize + a JPEG answer) equals the oracle chain on Pillow's pixels"""
    imp = gpu
    rng = np.random.default_rng(77)
    for il in (0, 1):
        blob, want = W.random_file(rng, 3, 8, il, 320, 200)
        frame = W.pillow(blob)
        assert np.array_equal(frame, want)
        rc, im = imp.Image.decode_png_ex(blob, imp.PNG_ALL)
        assert rc == 0
        cfg = imp.Config()
        rc, step = imp.run_ops(im, cfg, resize="160,0")
        assert rc == 0, (rc, step)
        rc, answer = im.encode_jpeg(86)
        rc_o, _, small = oracle_chain(frame, resize="160,0")
        assert rc_o == 0
        assert np.array_equal(im.numpy(), small)
        assert rc == 0 and answer == O.jpeg_encode(small, 86)[1]
        im.release()
