"""GIF albums and FreeImage frames through a real broker (protocol version 3, include/impgpu_broker.h): the pages of a GIF go in
as IMPB_IN_GIF and are composed in the broker -- all GIFs of a batch in one launch -- LoadSingle's bits go in as IMPB_IN_FI32;
every frame comes back (IMPB_OUT_FRAME) or leaves as FreeImage bitmaps (IMPB_OUT_FI).  Expected pixels are the oracle's."""
import os
import sys
import threading

import numpy as np
import pytest

import oracle_lib as orc
from conftest import ROOT, noise_image
from test_gif import random_album
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))
INVALID, MALLOC_FAILED, STEP_DECODE, STEP_ENCODE = 50, 2, 2, 8


@pytest.fixture(scope="module")
def served():
    """One broker for the module: slots of 2 MB (an album that does not fit is a small one), a gather window so that requests
    submitted together ride together.  It must stop with exit status 0 after everything the tests sent it."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(ROOT, "ngx_http_imgproc_amd", "build.py")], stdout=subprocess.DEVNULL)
    import worker_scaling
    from ngx_http_imgproc_amd import broker as B
    name = "/impgpu-test-album-%d" % os.getpid()
    p = worker_scaling.start_broker(name, threads=2, gather_us=20000, slots=12, extra=["--slot-mb", "2"])
    yield B, name, p
    err = worker_scaling.stop_broker(p)
    assert p.returncode == 0, err[-800:]
    assert not os.path.exists("/dev/shm" + name)


@pytest.fixture(scope="module")
def gif():
    """37 x 23, five pages, and the oracle's frames for both walks"""
    pages = random_album(31, 5, 37, 23)
    want = {}
    for destructive in (False, True):
        rc, frames = orc.gif_compose(pages, destructive)
        assert rc == 0 and len(frames) == 5
        want[destructive] = frames
    return pages, want


def per_frame(frames, **chain):
    out = []
    for f in frames:
        rc, _, got = oracle_chain(f, **chain)
        assert rc == 0
        out.append(got)
    return out


def same(got, want):
    return isinstance(got, list) and len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("destructive", [False, True])
def test_every_frame_of_a_gif_comes_back(served, gif, destructive):
    B, name, _ = served
    from ngx_http_imgproc_amd._lib import CConfig
    pages, want = gif
    frames = want[destructive]
    c = B.Client(name)
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=destructive, out=B.OUT_FRAME)
    assert (rc, code) == (0, 0) and a.frames == 5 and a.frame_stride >= 37 * 4 * 23 and same(got, frames)
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=destructive, resize="20,0", simple=1, out=B.OUT_FRAME)
    assert (rc, code) == (0, 0) and same(got, per_frame(frames, resize="20,0", simple=1))
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=destructive, crop="4,3", filters=["flip=10"], out=B.OUT_FRAME)
    assert (rc, code) == (0, 0) and same(got, per_frame(frames, crop="4,3", filters=["flip=10"]))
    ov = noise_image(6, 9, 4, 3)
    wid = c.prepare_watermark(ov)
    cfg = CConfig(2000, 2000, 5, 0, 60, b"r", b"b", 2, 1, None)
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=destructive, config=cfg, watermark_id=wid, out=B.OUT_FRAME)
    assert (rc, code) == (0, 0) and same(got, per_frame(frames, overlay=ov, wm=("r", "b", 2, 1, 60)))
    c.close()


def test_one_page_and_the_exits_that_mean_frame_zero(served, gif):
    B, name, _ = served
    pages, want = gif
    c = B.Client(name)
    rc, code, step, got, a = c.run(gif_pages=pages, page=2, out=B.OUT_FRAME)
    rc_o, one = orc.gif_compose(pages, False, 2)
    assert (rc, code, rc_o) == (0, 0, 0) and a.frames == 1 and np.array_equal(got, one[0])
    first = want[True][0]
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=1, out=B.OUT_INFO)
    assert (rc, code) == (0, 0) and (a.width, a.height) == (37, 23) and abs(a.brightness - orc.brightness(first)) < 1e-6
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=1, out=B.OUT_ASCII, ascii_args="")
    assert (rc, code) == (0, 0) and got == orc.ascii_art(first, "")
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=1, need_flatten=1, out=B.OUT_JPEG, quality=77)
    rc_o, _, flat = oracle_chain(first, flatten=1)
    rc_e, want_file = orc.jpeg_encode(flat, 77)
    assert (rc, code, rc_o, rc_e) == (0, 0, 0, 0) and got == want_file
    c.close()


@pytest.mark.parametrize("bpp", [24, 32])
def test_freeimage_bits_in_freeimage_bitmaps_out(served, gif, bpp):
    B, name, _ = served
    frame = noise_image(3, 5, 4, 80)                                  # what LoadSingle makes of the bitmap: top-down B,G,R,A
    bits = np.ascontiguousarray(frame[::-1]).reshape(3, 20)           # the bitmap itself: bottom-up, pitch 20
    assert np.array_equal(orc.fi32_to_ipl(bits, 5, 3), frame)
    c = B.Client(name)
    tight = 5 * bpp // 8
    rc, code, step, got, a = c.run(fi32=bits, out=B.OUT_FI, quality=bpp)
    want = orc.ipl_to_fi(frame, bpp)
    assert (rc, code) == (0, 0) and a.frames == 1 and (a.width, a.height, a.channels, a.row_step) == (5, 3, bpp // 8, want.shape[1])
    assert np.array_equal(got[0][:, :tight], want[:, :tight])
    # a bitmap with a pitch of its own and an operator in between
    wide = np.full((3, 28), 0xEE, np.uint8)
    wide[:, :20] = bits
    rc, code, step, got, a = c.run(fi32=(wide, 5), filters=["flip=10"], out=B.OUT_FI, quality=bpp)
    rc_o, _, flipped = oracle_chain(frame, filters=["flip=10"])
    assert (rc, code, rc_o) == (0, 0, 0) and np.array_equal(got[0][:, :tight], orc.ipl_to_fi(flipped, bpp)[:, :tight])
    # every frame of an album as FreeImage bitmaps (SaveGIF's per-frame IplToFI32)
    pages, frames = gif
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=1, out=B.OUT_FI, quality=bpp)
    assert (rc, code) == (0, 0) and a.frames == 5
    for g, f in zip(got, frames[True]):
        w = orc.ipl_to_fi(f, bpp)
        assert g.shape == w.shape and np.array_equal(g[:, :37 * bpp // 8], w[:, :37 * bpp // 8])
    rc, code, step, got, a = c.run(fi32=bits, out=B.OUT_FI, quality=16)
    assert rc == 0 and code == INVALID
    c.close()


def test_gifs_and_files_submitted_together_share_a_batch(served):
    B, name, _ = served
    albums = [(random_album(40 + i, 2 + i, 20 + 7 * i, 9 + 5 * i), bool(i & 1)) for i in range(6)]
    blobs = [orc.jpeg_encode(noise_image(40 + 8 * i, 56, 3, 90 + i), 90)[1] for i in range(2)]
    asks = [dict(gif_pages=p, destructive=d, resize="16,0", simple=1, out=B.OUT_FRAME) for p, d in albums] + \
           [dict(blob=b, resize="24,0", out=B.OUT_FRAME) for b in blobs]
    clients = [B.Client(name) for _ in asks]
    alone = [c.run(**ask) for c, ask in zip(clients, asks)]
    for (pages, d), r in zip(albums, alone[:6]):
        rc_o, frames = orc.gif_compose(pages, d)
        assert r[:2] == (0, 0) and rc_o == 0 and same(r[3], per_frame(frames, resize="16,0", simple=1))
    for b, r in zip(blobs, alone[6:]):
        rc_o, _, want = oracle_chain(orc.jpeg_decode(b)[1], resize="24,0")
        assert r[:2] == (0, 0) and rc_o == 0 and np.array_equal(r[3], want)
    together = [None] * len(asks)
    gate = threading.Barrier(len(asks))

    def ask_one(i):
        gate.wait()
        together[i] = clients[i].run(**asks[i])
    threads = [threading.Thread(target=ask_one, args=(i,)) for i in range(len(asks))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    for lone, r in zip(alone, together):
        assert r[:2] == (0, 0)
        assert same(r[3], lone[3]) if isinstance(lone[3], list) else np.array_equal(r[3], lone[3])
    assert max(r[4].batch_size for r in together) > 1, [r[4].batch_size for r in together]
    for c in clients:
        c.close()


def test_records_that_point_past_the_input_are_refused_and_the_broker_stays(served, gif):
    B, name, p = served
    pages, want = gif
    c = B.Client(name)
    rc, nbytes = c.pack_gif(pages)
    assert rc == 0
    buf = c.input_buffer(nbytes)
    good = B.CGifRecord.from_buffer_copy(bytes(buf[:48]))
    for field, value in (("indices_at", nbytes - good.pitch * good.height + 1), ("indices_at", 2 ** 64 - 8), ("palette_at", nbytes - 1023),
                         ("pitch", good.width - 1), ("height", -1)):
        rec = B.CGifRecord.from_buffer_copy(bytes(good))
        setattr(rec, field, value)
        buf[:48] = np.frombuffer(bytes(rec), np.uint8)                 # written straight into the input buffer
        rc, code, step, got, a = c.run(packed=(nbytes, len(pages)), out=B.OUT_FRAME)
        assert (rc, code, step) == (0, INVALID, STEP_DECODE) and a.bytes == 0, (field, rc, code, step)
    for count, pg in ((0, -1), (4097, -1), (len(pages), -2)):
        rc, code, step, got, a = c.run(packed=(nbytes, count), page=pg, out=B.OUT_FRAME)
        assert (rc, code, step) == (0, INVALID, STEP_DECODE), (count, pg)
    buf[:48] = np.frombuffer(bytes(good), np.uint8)
    rc, code, step, got, a = c.run(packed=(nbytes, len(pages)), out=B.OUT_FRAME)        # the same input, mended: served
    assert (rc, code) == (0, 0) and same(got, want[False]) and p.poll() is None
    c.close()


def test_an_album_that_does_not_fit_the_slot_is_said_so(served):
    """400 x 300 x 5 pages: 0.6 MB of pages go in, 2.4 MB of frames would have to come back through a slot of 2 MB -- the code an
    oversized answer always had.  One page of the same file fits and is served."""
    B, name, p = served
    rng = np.random.default_rng(3)
    from test_gif import page, palette
    pages = [page(rng.integers(0, 256, (300, 400), dtype=np.uint8), dispose=f % 3, key=f, pal=palette(9)) for f in range(5)]
    c = B.Client(name)
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=1, out=B.OUT_FRAME)
    assert (rc, code, step) == (0, MALLOC_FAILED, STEP_ENCODE) and "does not fit" in (a.error or b"").decode()
    # two frames fit as they are (0.96 MB behind 0.24 MB of pages) and no longer once an enlargement has doubled them
    rc, code, step, got, a = c.run(gif_pages=pages[:2], destructive=1, resize="800,0,up", simple=1, out=B.OUT_FRAME)
    assert (rc, code, step) == (0, MALLOC_FAILED, STEP_ENCODE)
    rc, code, step, got, a = c.run(gif_pages=pages, page=4, out=B.OUT_FRAME)
    rc_o, one = orc.gif_compose(pages, True, 4)
    assert (rc, code, rc_o) == (0, 0, 0) and np.array_equal(got, one[0]) and p.poll() is None
    c.close()
