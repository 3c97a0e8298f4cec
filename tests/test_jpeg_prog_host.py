"""Progressive JPEG, host side (no GPU): the multi-scan marker walk, the progression checks and the four scan decoders.
impgpu_jpeg_coefficients_ex(how = 0) is a plain bit-by-bit decoder of the file, (how = 1) runs the device's items with the
lanes' own code (csrc/imp_jpeg_prog.h); both must give the oracle's coefficients of the sequential twin -- for Pillow's
files (tests/golden/jpeg_prog) and for the files tests/jpeg_prog_writer.py writes, which reach what Pillow never writes.
"""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

import jpeg_prog_writer as W
import oracle_lib as orc

import ngx_http_imgproc_amd as imp
from ngx_http_imgproc_amd._lib import lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "jpeg_prog")
OLD = os.path.join(HERE, "golden", "jpeg")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
EXPECTED = np.load(os.path.join(GOLD, "expected_pixels.npz"))
NAMES = [c["name"] for c in MANIFEST["cases"]]
OLD_NAMES = [c["name"] for c in json.load(open(os.path.join(OLD, "manifest.json")))["cases"]]
P = imp.JPEG_PROGRESSIVE
# the baseline fixtures the writer's files are made of: gray, 4:4:4, 4:2:2, 4:2:0, sizes that are not MCU multiples, 1 x 1
WRITER_SOURCES = ["gray_q90_57x43", "c444_q90_48x40", "c422_q85_49x37", "c420_q90_67x45", "c420_q30_noise_64x64", "c420_q90_1x1", "c420_q90_5x17"]


def fixture(name, kind):
    with open(os.path.join(GOLD, "%s.%s.jpg" % (name, kind)), "rb") as f:
        return f.read()


def old_fixture(name):
    with open(os.path.join(OLD, name + ".jpg"), "rb") as f:
        return f.read()


def coefficients_ex(blob, how, accept=P):
    out = np.zeros(4_000_000, dtype=np.int16)
    info = (C.c_int * 12)()
    rc = lib.impgpu_jpeg_coefficients_ex(blob, len(blob), how, accept, out.ctypes.data, out.size, info)
    return rc, out[: info[0]].copy(), list(info)


def oracle_coefficients(blob):
    rc, info = orc.jpeg_info(blob)
    assert rc == 0
    return np.concatenate([orc.jpeg_coefficients(blob, ci)[1].reshape(-1) for ci in range(info["components"])])


def pillow_bgr(blob):
    Image = pytest.importorskip("PIL.Image")
    a = np.asarray(Image.open(io.BytesIO(blob)))
    return a[:, :, None] if a.ndim == 2 else a[:, :, ::-1]


def written_cases():
    """(id, source fixture, script name) for every legal script on every source"""
    return [("%s-%s" % (src, name), src, name) for src in WRITER_SOURCES for name in sorted(W.LEGAL)]


def expected_planes(src, script):
    """The source's coefficients as a decoder of the written file holds them: a scan of ONE component walks the component's
    own block grid, so the MCU-padding blocks of a component whose DC scan is not interleaved stay zero (libjpeg's arrays
    hold zeros there too; no pixel is made of them) -- an interleaved DC scan gives them the DC the encoder put there."""
    s = W.Source(old_fixture(src))
    planes = []
    for ci in range(s.ncomp):
        rc, c = orc.jpeg_coefficients(old_fixture(src), ci)
        c = c.copy()
        first_dc = [sc for sc in W.LEGAL[script](s.ncomp) if sc["ss"] == 0 and sc["ah"] == 0 and ci in sc["comps"]][0]
        if s.ncomp > 1 and len(first_dc["comps"]) == 1:
            rows, cols = s.grid[ci]
            c[rows:] = 0
            c[:, cols:] = 0
        planes.append(c.reshape(-1))
    return np.concatenate(planes)


def damaged_files(name):
    """seeded truncations and bit flips of a progressive fixture"""
    src = fixture(name, "prog")
    rng = np.random.Generator(np.random.PCG64(23))
    cases = [src[:cut] for cut in (3, 30, 200, len(src) // 2, len(src) - 10, len(src) - 2, len(src) - 1)]
    for _ in range(120):
        b = bytearray(src)
        for _ in range(int(rng.integers(1, 3))):
            b[int(rng.integers(2, len(b)))] ^= 1 << int(rng.integers(0, 8))
        cases.append(bytes(b))
    return cases


_written = {}


def written(src, script):
    if (src, script) not in _written:
        s = W.Source(old_fixture(src))
        _written[(src, script)] = W.write(s, W.LEGAL[script](s.ncomp))
    return _written[(src, script)]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("how", [0, 1], ids=["reference", "lane-code"])
def test_pillows_progressive_files_hold_their_twins_coefficients(name, how):
    blob, twin = fixture(name, "prog"), fixture(name, "seq")
    rc, got, info = coefficients_ex(blob, how)
    assert rc == 0 and info[1] == 0
    assert np.array_equal(got, oracle_coefficients(twin))
    case = MANIFEST["cases"][NAMES.index(name)]
    h, w, c = case["shape"]
    assert imp.jpeg_info_ex(blob, P) == (0, (w, h, c))
    assert info[2] == 3                                               # libjpeg's scripts, colour and gray: three levels
    # and without the bit everything is as before
    assert imp.jpeg_info_ex(blob, 0)[0] == imp.IMP_ERROR_UNSUPPORTED and imp.jpeg_info(blob)[0] == imp.IMP_ERROR_UNSUPPORTED
    assert coefficients_ex(blob, how, 0)[0] == imp.IMP_ERROR_UNSUPPORTED
    assert lib.impgpu_jpeg_classify(blob, len(blob)) == 1


@pytest.mark.parametrize("case", written_cases(), ids=[c[0] for c in written_cases()])
def test_written_files_hold_the_sources_coefficients(case):
    _, src, script = case
    blob = written(src, script)
    want = expected_planes(src, script)
    for how in (0, 1):
        rc, got, info = coefficients_ex(blob, how)
        assert rc == 0 and info[1] == 0, (how, rc, info[:3])
        assert np.array_equal(got, want), how


@pytest.mark.parametrize("case", written_cases(), ids=[c[0] for c in written_cases()])
def test_the_writer_itself_against_pillow(case):
    """Pillow decodes every legal written file to the pixels of the baseline file it was made of"""
    _, src, script = case
    assert np.array_equal(pillow_bgr(written(src, script)), pillow_bgr(old_fixture(src)))


def test_levels_follow_the_script():
    s = W.Source(old_fixture("c420_q90_67x45"))
    levels = {}
    for name in W.LEGAL:
        blob = W.write(s, W.LEGAL[name](3))
        rc, _, info = coefficients_ex(blob, 1)
        assert rc == 0
        levels[name] = info[2]
    assert levels["dc_then_full_ac"] == 1 and levels["dc_not_interleaved"] == 1 and levels["band_per_scan"] == 1
    assert levels["al_chain_3"] == 4 and levels["dri_changes"] == 2


@pytest.mark.parametrize("src", ["gray_q90_57x43", "c420_q90_67x45"])
def test_refusals_at_the_header(src):
    s = W.Source(old_fixture(src))
    for name, script in W.illegal_scripts(s.ncomp).items():
        blob = W.write(s, script)
        assert imp.jpeg_info_ex(blob, P)[0] == imp.IMP_ERROR_UNSUPPORTED, name
        for how in (0, 1):
            assert coefficients_ex(blob, how)[0] == imp.IMP_ERROR_UNSUPPORTED, name
    # a DQT behind the first scan, 12-bit samples and arithmetic coding stay refused with the bit set; no EOI is damage
    blob = written(src, "dc_then_full_ac")
    sos2 = blob.index(b"\xff\xda", blob.index(b"\xff\xda") + 2)
    dqt = blob[blob.index(b"\xff\xdb"):]
    dqt = dqt[: 2 + int.from_bytes(dqt[2:4], "big")]
    dht = blob.rindex(b"\xff\xc4", 0, sos2)
    assert imp.jpeg_info_ex(blob[:dht] + dqt + blob[dht:], P)[0] == imp.IMP_ERROR_UNSUPPORTED
    sof = blob.index(b"\xff\xc2")
    assert imp.jpeg_info_ex(blob[:sof + 4] + b"\x0c" + blob[sof + 5:], P)[0] == imp.IMP_ERROR_UNSUPPORTED
    assert imp.jpeg_info_ex(blob[:sof + 1] + b"\xca" + blob[sof + 2:], P)[0] == imp.IMP_ERROR_UNSUPPORTED
    assert imp.jpeg_info_ex(blob[:-2], P)[0] == imp.IMP_ERROR_DECODE_FAILED


def test_damaged_entropy_data_is_decode_failed():
    blob = fixture("c420_q90_dri4_95x51", "prog")
    first = blob.index(b"\xff\xda")
    data = first + 2 + int.from_bytes(blob[first + 2:first + 4], "big")
    # a byte of data behind the first interval's last block; a wrong RSTn; an interval cut short
    rst = blob.index(b"\xff\xd0", data)
    for bad in (blob[:rst] + b"\x55" + blob[rst:], blob[:rst + 1] + b"\xd3" + blob[rst + 2:], blob[:rst - 1] + blob[rst:]):
        for how in (0, 1):
            assert coefficients_ex(bad, how)[0] == imp.IMP_ERROR_DECODE_FAILED, how


@pytest.mark.parametrize("name", ["c420_q90_dri4_95x51", "gray_q90_57x43", "c444_q100_noise_64x48", "c422_q85_49x37"])
def test_truncations_and_flips_end_in_a_refusal_or_in_one_answer(name):
    """Never anything else: a damaged file is refused (UNSUPPORTED / DECODE_FAILED) by both decoders alike, or taken by
    both with the same coefficients.  (That the frame made of them is Pillow's is checked where frames are made:
    tests/test_gpu_jpeg_prog.py runs the same damaged files on the device.)"""
    taken = 0
    for b in damaged_files(name):
        rc0, got0, _ = coefficients_ex(b, 0)
        rc1, got1, _ = coefficients_ex(b, 1)
        assert rc0 in (0, imp.IMP_ERROR_UNSUPPORTED, imp.IMP_ERROR_DECODE_FAILED) and rc1 == rc0, (rc0, rc1)
        if rc0 == 0:
            taken += 1
            assert np.array_equal(got0, got1)
    assert taken > 5


@pytest.mark.parametrize("name", OLD_NAMES + [n + ".seq" for n in NAMES] + [n + ".prog" for n in NAMES])
def test_accept_zero_and_sequential_files_are_the_old_calls(name):
    if name.endswith((".seq", ".prog")):
        base, kind = name.rsplit(".", 1)
        blob = fixture(base, kind)
    else:
        blob = old_fixture(name)
    for accept in (0, P):
        if accept and name.endswith(".prog"):
            continue
        (rc_new, dims_new), (rc_old, dims_old) = imp.jpeg_info_ex(blob, accept), imp.jpeg_info(blob)
        assert rc_new == rc_old and (rc_old != 0 or dims_new == dims_old)
        for how in (0, 1):
            out = np.zeros(4_000_000, dtype=np.int16)
            info = (C.c_int * 12)()
            rc = lib.impgpu_jpeg_coefficients(blob, len(blob), how, out.ctypes.data, out.size, info)
            rc2, got2, info2 = coefficients_ex(blob, how, accept)
            assert rc == rc2
            if rc == 0:
                assert np.array_equal(out[: info[0]], got2) and list(info)[:2] == info2[:2]
