"""The host side of protocol version 3 (include/impgpu_broker.h): GIF pages and FreeImage bits through the broker.  No GPU:
the records stay one page each, the client's packing of a GIF's pages is read back out of the slot, and the broker's check
of such a request (csrc/imp_broker_check.h) runs under the sanitizers against a slow check written here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as orc
from conftest import ROOT
from test_gif import page, palette

INCLUDE = os.path.join(ROOT, "include")
INVALID, MALLOC_FAILED = 50, 2


@pytest.fixture(scope="module")
def built():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "ngx_http_imgproc_amd", "build.py")], stdout=subprocess.DEVNULL)
    from ngx_http_imgproc_amd import broker as B
    return B


def test_records_are_still_pages_and_the_new_fields_lie_in_front_of_the_error_text(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <impgpu_broker.h>\n#include <stddef.h>\n#include <stdio.h>\n'
                   'int main(void){printf("%zu %zu %zu %d %d\\n", sizeof(impb_header), sizeof(impb_slot), sizeof(impb_gif_page),\n'
                   ' offsetof(impb_slot_fields, out_frame_stride) + 8 <= offsetof(impb_slot_fields, error),\n'
                   ' offsetof(impb_slot_fields, in_pages) > offsetof(impb_slot_fields, broker_us));return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["4096", "4096", "48", "1", "1"]
    hdr = open(os.path.join(INCLUDE, "impgpu_broker.h")).read()
    assert "#define IMPB_VERSION      3u" in hdr and "#define IMPB_MAX_GIF_PAGES 4096" in hdr


# ---- impgpu_client_pack_gif against tests/c/album_mock.c, which answers a request with its own input
@pytest.fixture()
def mock(built, tmp_path):
    exe = str(tmp_path / "album_mock")
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, os.path.join(ROOT, "tests", "c", "album_mock.c"), "-o", exe, "-lrt"])
    name = "/impgpu-album-mock-%d" % os.getpid()
    p = subprocess.Popen([exe, name, "2", "64"], stdout=subprocess.PIPE, text=True)
    assert p.stdout.readline().strip() == "ready"
    yield name
    p.terminate()
    p.wait(timeout=30)
    assert not os.path.exists("/dev/shm" + name)


def some_pages():
    """Pitches of every kind: FreeImage's own (the 4-byte multiple that holds the row), a wider one (re-pitched), one equal
    to a width that is no multiple of 4 (kept: the walk's read past the row must land where it did); palettes shared."""
    rng = np.random.default_rng(5)
    a, b = palette(1), palette(2)
    def idx(h, w):
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    return [page(idx(6, 9), pal=a, key=3, dispose=1),
            page(idx(3, 5), left=2, top=1, pal=a, key=-1, dispose=2, pitch=14, pad_value=201),
            page(idx(4, 7), left=-1, top=3, pal=b, key=255, dispose=3, pitch=7),
            page(idx(2, 8), left=3, top=-1, pal=a, key=0, dispose=0, pad_value=9),
            page(idx(5, 4), left=6, top=2, pal=b, key=17, dispose=1, pitch=4)]


def parse(B, buf, count):
    """the records in the slot -> page dicts as the compose calls take them, and the palette offsets"""
    recs = [B.CGifRecord.from_buffer_copy(bytes(buf[i * 48:(i + 1) * 48])) for i in range(count)]
    pages = []
    for r in recs:
        assert r.indices_at + r.pitch * r.height <= len(buf) and r.palette_at + 1024 <= len(buf) and r.indices_at >= count * 48
        pages.append({"indices": np.array(buf[r.indices_at:r.indices_at + r.pitch * r.height]).reshape(r.height, r.pitch), "width": r.width,
                      "left": r.left, "top": r.top, "dispose": r.dispose, "key": r.transparency_key,
                      "palette": np.array(buf[r.palette_at:r.palette_at + 1024]).reshape(256, 4)})
    return pages, [r.palette_at for r in recs]


def test_pack_gif_round_trip(built, mock):
    B = built
    c = B.Client(mock)
    pages = some_pages()
    rc, nbytes = c.pack_gif(pages)
    assert rc == 0 and 5 * 48 + 2 * 1024 < nbytes < 5 * 48 + 2 * 1024 + 5 * 16 + sum(p["indices"].size for p in pages)
    buf = c.input_buffer(nbytes)
    back, pal_at = parse(B, buf, len(pages))
    for p, q in zip(pages, back):
        w, h = p["width"], p["indices"].shape[0]
        assert (q["width"], q["indices"].shape[0]) == (w, h)
        assert q["indices"].shape[1] <= max(p["indices"].shape[1], (w + 4) & ~3)
        assert np.array_equal(q["indices"][:, :w], p["indices"][:, :w])                    # every row, in FreeImage's order
        if p["indices"].shape[1] > w:
            assert np.array_equal(q["indices"][:, w], p["indices"][:, w])                  # the byte the walk reads at x == left + w
        assert [q[k] for k in ("left", "top", "dispose", "key")] == [p[k] for k in ("left", "top", "dispose", "key")]
        assert np.array_equal(q["palette"], p["palette"])
    assert len(set(pal_at)) == 2 and pal_at[0] == pal_at[1] == pal_at[3] and pal_at[2] == pal_at[4]     # a shared palette is stored once
    assert back[1]["indices"].shape[1] == 8 and back[2]["indices"].shape[1] == 7 and back[4]["indices"].shape[1] == 4
    # what counts: composing what the slot holds is composing the pages themselves
    for destructive, pg in ((False, -1), (True, -1), (False, 3)):
        rc_a, a = orc.gif_compose(pages, destructive, pg)
        rc_b, b = orc.gif_compose(back, destructive, pg)
        assert rc_a == rc_b == 0 and all(np.array_equal(x, y) for x, y in zip(a, b))
    packed = bytes(buf)
    # the same through impgpu_client_run: request.pages are packed on the way, the slot's GIF fields carry the rest
    rc, code, step, got, a = c.run(gif_pages=pages, destructive=1, page=2)
    assert (rc, code) == (0, 0) and got == packed and (a.width, a.height, a.channels, a.row_step) == (5, 2, 1, B.IN_GIF) and a.frames == 1
    # ... and packed ahead of time, as a caller does whose pages do not live until the round trip
    assert c.pack_gif(pages) == (0, nbytes)
    rc, code, step, got, a = c.run(packed=(nbytes, len(pages)), destructive=0, page=-1)
    assert (rc, code) == (0, 0) and got == packed and (a.width, a.height, a.channels) == (5, -1, 0)
    # an older caller's request is what it was
    rc, code, step, got, a = c.run(blob=b"abc")
    assert (rc, code) == (0, 0) and got == b"abc" and (a.width, a.height, a.channels, a.row_step) == (0, 0, 0, B.IN_FILE) and a.frames == 1
    c.close()


def test_pack_gif_refuses_what_does_not_fit_or_is_no_page(built, mock):
    B = built
    c = B.Client(mock)
    big = [page(np.zeros((300, 300), np.uint8))]                       # 90 KB of indices, slots of 64 KB
    assert c.pack_gif(big)[0] == MALLOC_FAILED
    assert c.run(gif_pages=big)[0] == MALLOC_FAILED
    fits = [page(np.zeros((100, 100), np.uint8))] * 6                  # 6 x 10 KB and one palette: fits; a seventh does not
    assert c.pack_gif(fits)[0] == 0 and c.pack_gif(fits + fits[:1])[0] == MALLOC_FAILED
    assert c.pack_gif([])[0] == INVALID
    bad = dict(some_pages()[0])
    bad["width"] = bad["indices"].shape[1] + 1                         # pitch < width
    assert c.pack_gif([bad])[0] == INVALID and c.run(gif_pages=[bad])[0] == INVALID
    assert c.stats()["served"] == 0                                    # nothing of all this was sent
    c.close()


# ---- csrc/imp_broker_check.h under the sanitizers
OK, BAD, TOO_LARGE = 0, 1, 2


def slow_check(slot_bytes, in_bytes, in_pages, in_page, recs):
    """The protocol's rules (impgpu_broker.h) in unbounded integers."""
    if in_bytes > slot_bytes or not 1 <= in_pages <= 4096 or in_page < -1 or in_pages * 48 > in_bytes:
        return BAD
    assert len(recs) == in_pages
    for indices_at, palette_at, w, h, pitch in recs:
        if w <= 0 or h <= 0 or pitch <= 0 or pitch < w:
            return BAD
        if indices_at + pitch * h > in_bytes or palette_at + 1024 > in_bytes:
            return BAD
    frames = 1 if in_page >= 0 else in_pages
    answer = frames * recs[0][2] * 4 * recs[0][3]
    if (in_bytes + 63) // 64 * 64 + answer > slot_bytes:
        return TOO_LARGE
    return OK


def test_the_brokers_check_of_gif_records_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "broker_check_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", INCLUDE, "-I", os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "broker_check_fuzz.cpp"), "-o", exe])
    seen = {OK: 0, BAD: 0, TOO_LARGE: 0}
    lines = 0
    for seed in (1, 2):
        r = subprocess.run([exe, "2000", str(seed)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
        for line in r.stdout.splitlines():
            v = [int(x) for x in line.split()]
            slot_bytes, in_bytes, in_pages, in_page, verdict, nrec = v[:6]
            recs = [tuple(v[6 + 5 * i:11 + 5 * i]) for i in range(nrec)]
            assert len(v) == 6 + 5 * nrec
            assert verdict == slow_check(slot_bytes, in_bytes, in_pages, in_page, recs), line[:200]
            seen[verdict] += 1
            lines += 1
    assert lines == 4000 and seen[OK] > 400 and seen[BAD] > 1200 and seen[TOO_LARGE] > 100, seen
