"""impgpu_*_decode_jpeg_ex with IMPGPU_JPEG_PROGRESSIVE on the device: every progressive fixture (Pillow's files,
tests/golden/jpeg_prog) and every legal file tests/jpeg_prog_writer.py writes decodes to libjpeg-turbo's pixels exactly,
alone and in one mixed batch with sequential, damaged and refused files; the two-halves and prepared forms give the same
frames; the level launches follow the scan script, not the file count; accept == 0 refuses as before; a decoded
progressive upload goes through the operator chain and the JPEG encoder like any other frame."""
import io
import os

import numpy as np
import pytest

import jpeg_prog_writer as W
import oracle_lib as orc
from conftest import ROOT
from test_gpu_chain import oracle_chain
from test_jpeg_prog_host import NAMES, WRITER_SOURCES, damaged_files, fixture, old_fixture, written, written_cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "jpeg_prog")
EXPECTED = np.load(os.path.join(GOLD, "expected_pixels.npz"))


def pixels(im):
    a = im.numpy()
    return a if a.ndim == 3 else a[:, :, None]


def single(imp, blob, accept):
    rc, im = imp.Image.decode_jpeg_ex(blob, accept)
    try:
        return rc, (pixels(im) if rc == 0 else None)
    finally:
        if im is not None:
            im.release()


def taken(res):
    out = []
    for rc, im in res:
        out.append((rc, pixels(im) if rc == 0 else None))
        if im is not None:
            im.release()
    return out


def source_pixels(src):
    rc, want = orc.jpeg_decode(old_fixture(src))
    assert rc == 0
    return want


def all_good_files():
    """(name, file, expected pixels): Pillow's fixtures, then every legal written file"""
    out = [(n, fixture(n, "prog"), EXPECTED[n]) for n in NAMES]
    out += [(cid, written(src, script), source_pixels(src)) for cid, src, script in written_cases()]
    return out


def test_every_progressive_file_alone(gpu):
    imp = gpu
    before = imp.jpeg_counters()
    good = all_good_files()
    for name, blob, want in good:
        rc, got = single(imp, blob, imp.JPEG_PROGRESSIVE)
        assert rc == 0, name
        assert got.shape == want.shape and np.array_equal(got, want), name
    after = imp.jpeg_counters()
    assert after[13] - before[13] == len(good) and after[5] == before[5]


def test_accept_zero_refuses_as_before(gpu):
    imp = gpu
    before = imp.jpeg_counters()
    for name in NAMES:
        blob = fixture(name, "prog")
        assert single(imp, blob, 0)[0] == imp.IMP_ERROR_UNSUPPORTED
        assert imp.Image.decode_jpeg(blob)[0] == imp.IMP_ERROR_UNSUPPORTED
        # the sequential twin through _ex, with and without the bit: the old call's frame
        twin = fixture(name, "seq")
        rc0, im0 = imp.Image.decode_jpeg(twin)
        assert rc0 == 0
        for accept in (0, imp.JPEG_PROGRESSIVE):
            rc, got = single(imp, twin, accept)
            assert rc == 0 and np.array_equal(got, pixels(im0))
        im0.release()
    res = taken(imp.batch_decode_jpeg([fixture(n, "prog") for n in NAMES]))
    assert all(rc == imp.IMP_ERROR_UNSUPPORTED for rc, _ in res)
    after = imp.jpeg_counters()
    assert after[5] - before[5] == 3 * len(NAMES) and after[13] == before[13] and after[14] == before[14]


def _mixed():
    """(file, expected code, expected pixels or None)"""
    s = W.Source(old_fixture("c420_q90_67x45"))
    illegal = W.illegal_scripts(3)
    dri = fixture("c420_q90_dri4_95x51", "prog")
    first = dri.index(b"\xff\xda")
    rst = dri.index(b"\xff\xd0", first)
    noise = fixture("c444_q100_noise_64x48", "prog")
    last = noise.rindex(b"\xff\xda")
    work = []
    for k, (name, blob, want) in enumerate(all_good_files()):
        work.append((blob, 0, want))
        if k % 5 == 0:                                               # sequential neighbours
            src = WRITER_SOURCES[(k // 5) % len(WRITER_SOURCES)]
            work.append((old_fixture(src), 0, source_pixels(src)))
        if k % 7 == 0:                                               # refused at the header
            key = sorted(illegal)[(k // 7) % len(illegal)]
            work.append((W.write(s, illegal[key]), 1, None))
        if k % 9 == 0:                                               # damaged entropy data, each in its own way
            bad = [dri[:rst] + b"\x55" + dri[rst:], dri[:rst - 1] + dri[rst:], noise[:last + 40] + noise[last + 90:],
                   dri[:rst + 1] + b"\xd5" + dri[rst + 2:]][(k // 9) % 4]
            work.append((bad, 3, None))
    work.append((b"\x89PNG\r\n\x1a\n" + b"\0" * 64, 1, None))
    return work


def test_one_mixed_batch(gpu):
    imp = gpu
    work = _mixed()
    assert len(work) > 60
    res = taken(imp.batch_decode_jpeg_ex([w[0] for w in work], imp.JPEG_PROGRESSIVE))
    for k, ((blob, code, want), (rc, got)) in enumerate(zip(work, res)):
        assert rc == code, k
        if code == 0:
            assert got.shape == want.shape and np.array_equal(got, want), k


def test_two_halves_prepared_and_pending_give_the_same_frames(gpu):
    imp = gpu
    work = _mixed()[:30]
    blobs = [w[0] for w in work]
    for kw in (dict(), dict(prepared=True), dict(prepared=True, pending=True)):
        res, _ = imp.batch_decode_jpeg_begin_finish_ex(blobs, imp.JPEG_PROGRESSIVE, **kw)
        for k, ((blob, code, want), (rc, got)) in enumerate(zip(work, taken(res))):
            assert rc == code, (kw, k)
            if code == 0:
                assert np.array_equal(got, want), (kw, k)
    # batches begun WITHOUT the bit finish as before
    res, launches = imp.batch_decode_jpeg_begin_finish_ex(blobs, 0)
    assert launches == 0
    for (blob, code, want), (rc, got) in zip(work, taken(res)):
        progressive = imp.lib.impgpu_jpeg_classify(blob, len(blob)) == 1
        assert rc == (1 if progressive else code)


def test_launches_follow_the_script_not_the_file_count(gpu):
    imp = gpu
    blob = fixture("c420_q90_67x45", "prog")
    want = EXPECTED["c420_q90_67x45"]
    counts = {}
    for n in (1, 32):
        before = imp.jpeg_counters()
        res, launches = imp.batch_decode_jpeg_begin_finish_ex([blob] * n, imp.JPEG_PROGRESSIVE)
        for rc, got in taken(res):
            assert rc == 0 and np.array_equal(got, want)
        counts[n] = launches
        assert imp.jpeg_counters()[14] - before[14] == launches
    assert counts[1] == counts[32] == 3                              # libjpeg's ten-scan script: three levels
    deep = written("c420_q90_67x45", "al_chain_3")
    res, launches = imp.batch_decode_jpeg_begin_finish_ex([deep, blob, old_fixture("c420_q90_67x45")] * 4, imp.JPEG_PROGRESSIVE)
    assert launches == 4 and all(rc == 0 for rc, _ in taken(res))    # the deepest script of the batch


@pytest.mark.parametrize("name", ["c420_q90_dri4_95x51", "gray_q90_57x43", "c444_q100_noise_64x48", "c422_q85_49x37"])
def test_damaged_files_are_refused_or_pillows(gpu, name):
    """truncations and bit flips: UNSUPPORTED / DECODE_FAILED, or exactly what Pillow shows -- never anything else; the good
    file riding the same batch is untouched"""
    Image = pytest.importorskip("PIL.Image")
    imp = gpu
    files = damaged_files(name)
    good, want_good = fixture(name, "prog"), EXPECTED[name]
    res = taken(imp.batch_decode_jpeg_ex(files + [good], imp.JPEG_PROGRESSIVE))
    assert res[-1][0] == 0 and np.array_equal(res[-1][1], want_good)
    compared = 0
    for b, (rc, got) in zip(files, res):
        assert rc in (0, imp.IMP_ERROR_UNSUPPORTED, imp.IMP_ERROR_DECODE_FAILED)
        if rc:
            continue
        a = np.asarray(Image.open(io.BytesIO(b)))
        a = a[:, :, None] if a.ndim == 2 else a[:, :, ::-1]
        assert np.array_equal(got, a)
        compared += 1
    assert compared > 5


def test_a_progressive_upload_through_the_operators_and_the_encoder(gpu):
    imp = gpu
    cfg = imp.Config(allow_experiments=True)
    for name in ("c420_q50_400x300", "gray_q75_640x480", "c444_q100_noise_64x48"):
        rc, im = imp.Image.decode_jpeg_ex(fixture(name, "prog"), imp.JPEG_PROGRESSIVE)
        assert rc == 0
        rc, step = imp.run_ops(im, cfg, crop="4,3", resize="160,0", filters=["gamma=1.4"])
        assert rc == 0, step
        rc, answer = im.encode_jpeg(86)
        im.release()
        rc_o, _, frame = oracle_chain(EXPECTED[name], crop="4,3", resize="160,0", filters=["gamma=1.4"])
        assert rc_o == 0
        rc_o, want = orc.jpeg_encode(frame, 86)
        assert rc == rc_o == 0 and answer == want, name


def test_photographs_found_on_the_box_through_ex(gpu):
    """tests/golden/jpeg/found through the _ex call with the bit set: a file that classifies as progressive must now equal
    Pillow, and the sequential ones still do.  (The folder's four files are all sequential: the one progressive file of
    DESIGN section 0 row 6's corpus is a vendor's logo and was never stored here.)"""
    Image = pytest.importorskip("PIL.Image")
    imp = gpu
    found = os.path.join(ROOT, "tests", "golden", "jpeg", "found")
    compared = 0
    for n in sorted(os.listdir(found)):
        if not n.endswith(".jpg"):
            continue
        blob = open(os.path.join(found, n), "rb").read()
        kind = imp.lib.impgpu_jpeg_classify(blob, len(blob))
        rc, got = single(imp, blob, imp.JPEG_PROGRESSIVE)
        if kind in (0, 1):
            im = Image.open(io.BytesIO(blob))
            assert im.mode in ("RGB", "L")
            want = np.asarray(im)
            want = want[:, :, ::-1] if want.ndim == 3 else want[:, :, None]
            assert rc == 0 and np.array_equal(got, want), n
            compared += 1
        else:
            assert rc in (imp.IMP_ERROR_UNSUPPORTED, imp.IMP_ERROR_DECODE_FAILED), n
    assert compared > 0
