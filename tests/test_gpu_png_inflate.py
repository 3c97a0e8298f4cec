"""IMPGPU_PNG_DEVICE_INFLATE on the device: k_png_inflate (one wavefront per zlib stream) in front of the unfilter and place
launches.  The bit selects how files are decoded, not which: codes and pixels are those of the same call without it (and
Pillow's); a damaged stream fails alone; *launches is the count without the bit plus one per group; the calls without the
bit launch what they launched before."""
import io
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

import inflate_cases as K
from conftest import ROOT
from png_writer import chunk, filter_rows, write_png

pytestmark = pytest.mark.gpu

EXT = os.path.join(ROOT, "tests", "golden", "png_ext")
EXT_MANIFEST = json.load(open(os.path.join(EXT, "manifest.json")))
DEV = 8


def pixels(im):
    a = im.numpy()
    return a if a.ndim == 3 else a[:, :, None]


def pillow(blob):
    a = np.asarray(Image.open(io.BytesIO(blob)))
    if a.ndim == 2:
        return a[:, :, None]
    return a[:, :, [2, 1, 0] + ([3] if a.shape[2] == 4 else [])]


def png_of(arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(b, "PNG", **kw)
    return b.getvalue()


def png_from_stream(z, w, h, colour=0, pieces=1):
    """a PNG whose IDAT chunks hold the zlib stream z, cut into `pieces`"""
    ihdr = struct.pack(">IIBBBBB", w, h, 8, colour, 0, 0, 0)
    cuts = [len(z) * i // pieces for i in range(pieces + 1)]
    body = b"".join(chunk(b"IDAT", z[cuts[i]:cuts[i + 1]]) for i in range(pieces))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + body + chunk(b"IEND", b"")


def batch(imp, blobs, accept):
    res, launches = imp.batch_decode_png_ex(blobs, accept)
    out = []
    for rc, im in res:
        out.append((rc, pixels(im).copy() if rc == 0 else None))
        if im is not None:
            im.release()
    return out, launches


def same(a, b):
    assert len(a) == len(b)
    for k, ((rca, pa), (rcb, pb)) in enumerate(zip(a, b)):
        assert rca == rcb, (k, rca, rcb)
        assert (pa is None) == (pb is None) and (pa is None or np.array_equal(pa, pb)), k


def mixed_files():
    from ngx_http_imgproc_amd.workloads import photo_like

    rng = np.random.default_rng(77)
    files = [png_of(np.full((1, 1, 1), 5, np.uint8)),
             png_of(rng.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)),
             png_of(photo_like(100, 128, 3), compress_level=6)]                       # 38.5 KB of scanlines: the ring wraps
    noise = rng.integers(0, 256, size=(140, 160, 3), dtype=np.uint8)
    files.append(write_png(noise, [int(v) for v in rng.integers(0, 5, size=140)], 2, level=0))      # 67 340 bytes: two stored blocks
    files.append(png_of(np.full((64, 200, 3), (9, 200, 31), np.uint8)))              # distance-1 runs
    gray = photo_like(200, 300, 5)[:, :, 1]
    z = K.compress(filter_rows(gray[:, :, None], [y % 5 for y in range(200)]), 6, sync_every=1000)
    files.append(png_from_stream(z, 300, 200, pieces=9))                             # many blocks, empty stored ones, 9 IDAT chunks
    files.append(png_from_stream(K.compress(K.rows_of(K.steep(70000), 3500), 6, zlib.Z_HUFFMAN_ONLY), 3499, 20))   # the longest codes
    files.append(png_from_stream(K.far_stream(40000, 200, 201)[0], 200, 200))        # distance 32 768, the ring wrapped
    return files


def test_a_mixed_call(gpu):
    imp = gpu
    files = mixed_files()
    assert len(zlib.decompress(b"".join(_idat(files[3])))) == 67340
    got, _ = batch(imp, files, DEV)
    want, _ = batch(imp, files, 0)
    for k, (blob, (rc, px)) in enumerate(zip(files, got)):
        assert rc == 0, k
        assert np.array_equal(px, pillow(blob)), k
    same(got, want)
    got_all, _ = batch(imp, files, imp.PNG_ALL | DEV)
    same(got_all, want)


def _idat(blob):
    at, out = 8, []
    while at < len(blob):
        n, kind = struct.unpack(">I4s", blob[at:at + 8])
        if kind == b"IDAT":
            out.append(blob[at + 8:at + 8 + n])
        at += 12 + n
    return out


def test_item_files(gpu):
    """palette, low-bit gray and Adam7 fixtures: the items' rows are checked and cleared, the palette reaches its region"""
    imp = gpu
    names = sorted(EXT_MANIFEST)
    blobs = [open(os.path.join(EXT, n), "rb").read() for n in names]
    got, launches_dev = batch(imp, blobs, imp.PNG_ALL | DEV)
    want, launches = batch(imp, blobs, imp.PNG_ALL)
    same(got, want)
    assert any(rc == 0 for rc, _ in want) and launches_dev == launches + 1
    for name, (rc, _) in zip(names, got):
        assert rc == EXT_MANIFEST[name]["code"], name


def damaged_files():
    from ngx_http_imgproc_amd.workloads import photo_like

    sound = [png_of(photo_like(60 + 7 * k, 90 + 5 * k, k), compress_level=6) for k in range(4)]
    base = png_of(photo_like(80, 100, 9), compress_level=6)
    z = b"".join(_idat(base))
    assert (z[2] >> 1) & 3 == 2                                                       # a dynamic block
    truncated = png_from_stream(z[:len(z) // 2], 100, 80, colour=2)
    flipped = bytearray(z)
    flipped[3] ^= 0x10                                                               # inside the dynamic block's header
    flipped = png_from_stream(bytes(flipped), 100, 80, colour=2)
    raw = bytearray(zlib.decompress(z))
    raw[79 * 301] = 5                                                                # the last row's filter byte
    filter5 = png_from_stream(zlib.compress(bytes(raw), 6), 100, 80, colour=2)
    trailing = png_from_stream(zlib.compress(zlib.decompress(z) + bytes(range(200)), 6), 100, 80, colour=2)
    return [sound[0], truncated, sound[1], flipped, filter5, sound[2], trailing, sound[3]]


def test_verdicts_inside_a_batch(gpu):
    imp = gpu
    files = damaged_files()
    got, _ = batch(imp, files, DEV)
    want, _ = batch(imp, files, 0)
    same(got, want)
    assert [rc for rc, _ in got] == [0, imp.IMP_ERROR_DECODE_FAILED, 0, imp.IMP_ERROR_DECODE_FAILED, imp.IMP_ERROR_DECODE_FAILED, 0, 0, 0]
    for k in (0, 2, 5, 6, 7):
        assert np.array_equal(got[k][1], pillow(files[k])), k
    # one damaged file next to one sound neighbour, the damaged one first and last
    for pair in ([files[1], files[0]], [files[0], files[3]], [files[4], files[2]]):
        got, _ = batch(imp, pair, DEV)
        want, _ = batch(imp, pair, 0)
        same(got, want)
        assert sorted(rc for rc, _ in got) == [0, imp.IMP_ERROR_DECODE_FAILED]


def test_guarded_destination_on_the_host():
    """the lanes' own stores, with canaries round the destination (the device's scanline regions cannot carry canaries: the
    same code runs here on the CPU) -- damaged and sound streams of this file's batch"""
    import ctypes as C

    import ngx_http_imgproc_amd as imp

    for blob in damaged_files()[:5]:
        z = b"".join(_idat(blob))
        n = 301 * 80 if len(z) > 100 else 1
        for size in (n, n - 7, n + 9):
            buf = np.full(size + 128, 0xA5, np.uint8)
            st = C.c_int(-1)
            imp.lib.impgpu_png_inflate_lanes(z, len(z), buf.ctypes.data + 64, size, C.byref(st))
            assert (buf[:64] == 0xA5).all() and (buf[64 + size:] == 0xA5).all()


def test_256_files_of_3_by_3(gpu):
    imp = gpu
    rng = np.random.default_rng(256)
    files = [png_of(rng.integers(0, 256, size=(3, 3, [1, 3, 4][k % 3]), dtype=np.uint8), compress_level=k % 10) for k in range(256)]
    got, launches = batch(imp, files, DEV)
    assert launches == 4
    for blob, (rc, px) in zip(files, got):
        assert rc == 0 and np.array_equal(px, pillow(blob))


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
    a = photo_like(480, 640, 100 + k)
    a = a[:, :, 1] if k % 3 == 0 else np.dstack([a, a[:, :, :1]]) if k % 3 == 1 else a
    Image.fromarray(a).save(b, "PNG", compress_level=1)
    blobs.append(b.getvalue())
out = {}
for accept in (0, 8):
    res, launches = imp.batch_decode_png_ex(blobs, accept)
    ok = 0
    for blob, (rc, im) in zip(blobs, res):
        want = np.asarray(Image.open(io.BytesIO(blob)))
        want = want[:, :, None] if want.ndim == 2 else want[:, :, [2, 1, 0] + ([3] if want.shape[2] == 4 else [])]
        got = im.numpy() if rc == 0 else None
        ok += int(rc == 0 and np.array_equal(got if got.ndim == 3 else got[:, :, None], want))
    del res, im
    out[str(accept)] = {"ok": ok, "launches": launches}
imp.env_destroy()
print(json.dumps(out))
"""


def test_launches_are_todays_plus_one_per_group(gpu):
    imp = gpu
    rng = np.random.default_rng(3)
    files = [png_of(rng.integers(0, 256, size=(30, 20 + i, c), dtype=np.uint8)) for c in (1, 3, 4) for i in range(4)]
    _, plain = batch(imp, files, 0)
    _, dev = batch(imp, files, DEV)
    assert plain == 3 and dev == plain + 1
    _, dev = batch(imp, files[:4], DEV)
    assert dev == 2
    # IMPGPU_STAGE_CAP_MB=9 in a fresh process (the cap is read once): twenty 640 x 480 files of 1 / 3 / 4 channels
    # (0.3 / 0.9 / 1.2 MB of scanlines) go in two groups, each of its own inflate launch
    env = dict(os.environ, IMPGPU_STAGE_CAP_MB="9")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["0"]["ok"] == 20 and r["8"]["ok"] == 20, r
    assert r["0"]["launches"] == 6 and r["8"]["launches"] == r["0"]["launches"] + 2, r


def test_the_lone_call(gpu):
    imp = gpu
    ext = [open(os.path.join(EXT, n), "rb").read() for n in sorted(EXT_MANIFEST)][:6]
    for blob in mixed_files()[:5] + damaged_files()[:5] + ext:
        for accept in (0, imp.PNG_ALL):
            rc0, im0 = imp.Image.decode_png_ex(blob, accept)
            rc1, im1 = imp.Image.decode_png_ex(blob, accept | DEV)
            assert rc0 == rc1
            assert (im0 is None) == (im1 is None) and (im0 is None or np.array_equal(im0.numpy(), im1.numpy()))
            for im in (im0, im1):
                if im is not None:
                    im.release()


def test_the_default_is_untouched(gpu):
    """without the bit: today's launches (one k_png_unfilter_batch per channel count; items: unfilter per filter unit + place
    per channel count) -- this one passes before the device inflate exists, and guards that it changed nothing"""
    imp = gpu
    rng = np.random.default_rng(3)
    files = [png_of(rng.integers(0, 256, size=(30, 20 + i, c), dtype=np.uint8)) for c in (1, 3, 4) for i in range(4)]
    for accept in (0, imp.PNG_ALL):
        got, launches = batch(imp, files, accept)
        assert launches == 3 and all(rc == 0 for rc, _ in got)
    res, launches = imp.batch_decode_png(files)
    assert launches == 3
    names = sorted(EXT_MANIFEST)
    blobs = [open(os.path.join(EXT, n), "rb").read() for n in names]
    _, launches = batch(imp, blobs, imp.PNG_ALL)
    assert launches <= 6
