"""INTER_AREA shrinks whose cells span 21..66 source columns, of the frames k_resize_area_wide and k_resize_area_wide_mix
fetch by COVERING granules: gray frames (any pointer, any pitch) and BGR frames off the 4-byte grid (a crop window that
starts at a column not divisible by 4, a pitch that is no multiple of 4).

Every output must equal, byte for byte, what one impgpu_batch_cv_resize launch per frame leaves and what the oracle computes
(itself pinned on these shapes by test_oracle_wide_area for colour and test_oracle_wide_area_gray for one channel); the
number of kernels enqueued must follow the kinds of frames in the call, not their number: such frames share the wide launch
of their channel count, the aligned BGR ones included."""
import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image, smooth_image
from test_gpu_batch_ops import Configs, Req, _release, check_against_loop, check_against_oracle, run_both
from test_gpu_gray_mix import widest_cell
from test_gpu_int_mix import CANARY, Frame, _check_frames, _general_frame
from test_gpu_wide_area import WideFrame
from test_oracle_wide_area_gray import ACCEPTED, OLD_PATH, PAST_RULE, W_MAX, W_MIN

pytestmark = pytest.mark.gpu

# where a source window lies.  Gray: (pointer % 16, pitch % 16) -- the offset of a row's segment inside its first granule
# is constant (pitch = 0 mod 16), walks by one a row (1), walks unevenly (5).  BGR: (pixels the window starts into a
# 4-byte aligned row, pitch a multiple of 4 or not) -- pointer % 4 = 3, 2, 1.  None: a tight frame, whose window starts
# the allocation and ends it (BGR: a shape with sw * 3 % 4 != 0 then has an off-grid pitch).
GRAY_PLACES = [(s, p) for s in (0, 1, 7, 15) for p in (0, 1, 5)] + [None]
BGR_PLACES = [(ox, al) for ox in (1, 2, 3) for al in (True, False)] + [None]
TIGHT_BGR = [s for s in ACCEPTED if (s[0] * 3) % 4]


def _places(cn):
    return GRAY_PLACES if cn == 1 else BGR_PLACES


class CoverFrame(Frame):
    """test_gpu_int_mix.Frame with a chosen source placement (above); the destination window lies at any alignment."""

    def __init__(self, torch, rng, cn, sw, sh, dw, dh, place):
        self.cn, self.sw, self.sh, self.dw, self.dh, self.interp = cn, sw, sh, dw, dh, orc.INTER_AREA
        py = int(rng.integers(0, 3))
        if place is None:
            ox, oy, py, pitch = 0, 0, 0, sw * cn
        elif cn == 1:
            shift, pm = place
            oy = int(rng.integers(1, 5))
            pitch = sw + 16 + (pm - (sw + 16)) % 16
            ox = (shift - oy * pitch) % 16
        else:
            ox, aligned = place
            oy = 4 * int(rng.integers(0, 2))                           # (rows start on the 4-byte grid whatever the pitch is)
            pitch = (sw + ox + int(rng.integers(0, 3))) * 3
            pitch += (-pitch) % 4 if aligned else (1 if (pitch + 1) % 4 else 2)
        flat = rng.integers(0, 256, size=((sh + oy + py) * pitch,), dtype=np.uint8)
        rows = flat.reshape(sh + oy + py, pitch)
        self.host = flat
        self.window = rows[oy:oy + sh, ox * cn:(ox + sw) * cn].reshape(sh, sw, cn)
        self.src = torch.from_numpy(flat).cuda()
        self.sstep = pitch
        self.sptr = self.src.data_ptr() + oy * pitch + ox * cn
        if place is not None and cn == 1:
            assert self.sptr % 16 == place[0] and pitch % 16 == place[1]
        elif place is not None:
            assert self.sptr % 4 == (3 * place[0]) % 4 != 0 and (pitch % 4 == 0) == place[1]
        else:
            assert self.src.numel() == sh * sw * cn
        dpad = int(rng.integers(0, 4))
        self.dsts = [torch.full((dh, dw + dpad, cn), CANARY, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.dstep = (dw + dpad) * cn


def _cover_frames(torch, rng, cn, shapes):
    return [CoverFrame(torch, rng, cn, *s, place=p) for s in shapes for p in _places(cn)
            if p is not None or cn == 1 or s in TIGHT_BGR]


def test_the_shapes_are_what_they_claim():
    assert len(ACCEPTED) == 8 and len(TIGHT_BGR) >= 1
    assert all(W_MIN <= widest_cell(sw, dw) <= W_MAX for sw, _, dw, _ in ACCEPTED)
    assert widest_cell(OLD_PATH[0], OLD_PATH[2]) == 20 and widest_cell(PAST_RULE[0], PAST_RULE[2]) == 67


# ---------------------------------------------------------------- 1. alone and in uniform batches
@pytest.mark.parametrize("cn", [1, 3])
def test_lone_launch(gpu, cn):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DA100 + cn))
    frames = _cover_frames(torch, rng, cn, ACCEPTED + [OLD_PATH, PAST_RULE])
    torch.cuda.synchronize()
    for f in frames:
        sp, sw, sh, ss, dp, dw, dh, ds = f.item(0)
        gpu.batch_cv_resize(sp, 0, sw, sh, ss, dp, 0, dw, dh, ds, cn, 1, orc.INTER_AREA)
    _check_frames(gpu, frames, cn, "lone")                             # (the oracle, the canaries; a second launch leaves the same)


# (pointer offset, pitch residue, frame-stride residue): gray mod 16, BGR mod 4.  An odd frame stride gives the nine frames
# of one call nine different pointer alignments.
BATCH_PLACES = {1: [(0, 0, 0), (7, 1, 3), (15, 5, 9)], 3: [(3, 0, 0), (6, 0, 2), (9, 1, 3)]}


@pytest.mark.parametrize("cn", [1, 3])
def test_uniform_batch_of_nine(gpu, cn):
    import torch

    count = 9                                                          # one full group of 8 frames and a padded one
    mod = 16 if cn == 1 else 4
    rng = np.random.Generator(np.random.PCG64(0x1A4DA200 + cn))
    for sw, sh, dw, dh in ACCEPTED:
        for start, pm, sm in BATCH_PLACES[cn]:
            pitch = sw * cn + 16 + (pm - (sw * cn + 16)) % mod
            stride = sh * pitch + (sm - sh * pitch) % mod
            dpad = int(rng.integers(0, 4))
            flat = rng.integers(0, 256, size=(start + count * stride,), dtype=np.uint8)
            src = torch.from_numpy(flat).cuda()
            dst = torch.full((count, dh, dw + dpad, cn), CANARY, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dstep = (dw + dpad) * cn
            gpu.batch_cv_resize(src.data_ptr() + start, stride, sw, sh, pitch, dst.data_ptr(), dh * dstep, dw, dh, dstep, cn, count,
                                orc.INTER_AREA)
            gpu.sync()
            got = dst.cpu().numpy()
            for k in range(count):
                window = flat[start + k * stride:start + k * stride + sh * pitch].reshape(sh, pitch)[:, :sw * cn].reshape(sh, sw, cn)
                want = orc.cv_resize(np.ascontiguousarray(window), dw, dh, orc.INTER_AREA).reshape(dh, dw, cn)
                assert np.array_equal(got[k, :, :dw], want), (cn, sw, sh, dw, dh, start, pm, sm, k)
            assert (got[:, :, dw:] == CANARY).all(), (cn, sw, sh, dw, dh)


# ---------------------------------------------------------------- 2. frames of different geometry, the direct API
def _mixed(gpu, frames, cn):
    import torch

    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, count_launches=True)
    assert rc == 0
    return launches


def _again(frames):
    for f in frames:
        f.dsts[0].fill_(CANARY)


def test_mixed_gray_call_shares_one_launch(gpu):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DA300))
    places = [GRAY_PLACES[(5 * i + 1) % len(GRAY_PLACES)] for i in range(len(ACCEPTED))]
    assert len(set(places)) == len(ACCEPTED)                           # every frame lies differently
    wide = [CoverFrame(torch, rng, 1, *s, place=p) for s, p in zip(ACCEPTED, places)]
    launches = _mixed(gpu, wide, 1)
    print("gray: %d wide frames, %d launches" % (len(wide), launches))
    _check_frames(gpu, wide, 1, "wide")
    assert launches == 1, launches                                     # (one k_resize_area<1> launch each before: 8)
    general = [_general_frame(torch, rng, 1) for _ in range(3)]
    whole = [Frame(torch, rng, 1, 4 * 60, 4 * 30, 60, 30, orc.INTER_AREA), Frame(torch, rng, 1, 3 * 50, 5 * 20, 50, 20, orc.INTER_AREA)]
    frames = wide[:5] + general[:2] + whole[:1] + wide[5:] + general[2:] + whole[1:]
    _again(frames)
    launches = _mixed(gpu, frames, 1)
    _check_frames(gpu, frames, 1, "mixed")
    assert launches == 3, launches                                     # wide cells, general shrinks, whole factors
    more = frames + [CoverFrame(torch, rng, 1, *PAST_RULE, place=(7, 5))]
    _again(frames)
    launches = _mixed(gpu, more, 1)
    _check_frames(gpu, more, 1, "mixed + past the rule")
    assert launches == 4, launches                                     # ... and the W = 67 frame alone, by its tables
    old = [CoverFrame(torch, rng, 1, *OLD_PATH, place=(1, 1)), CoverFrame(torch, rng, 1, *OLD_PATH, place=(15, 5))]
    launches = _mixed(gpu, old, 1)
    _check_frames(gpu, old, 1, "W = 20")
    assert launches == 1, launches                                     # as before: k_resize_area_mix<1>


def test_mixed_bgr_call_shares_one_launch(gpu):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DA400))
    aligned = [WideFrame(torch, rng, 3, *s) for s in ACCEPTED[:4]]
    off_grid = [CoverFrame(torch, rng, 3, *s, place=p) for s, p in zip(ACCEPTED[4:], [(1, True), (2, False), (3, True), (3, False)])]
    frames = [f for pair in zip(aligned, off_grid) for f in pair]
    launches = _mixed(gpu, frames, 3)
    print("BGR: %d aligned and %d off-grid frames, %d launches" % (len(aligned), len(off_grid), launches))
    _check_frames(gpu, frames, 3, "aligned + off-grid")
    assert launches == 1, launches                                     # (before: the aligned four in one, the others one each: 5)


# ---------------------------------------------------------------- 3. a fuzz
FUZZ_SEEDS = range(6)


def fuzz_geometries(seed, cn):
    """The frames of one fuzz call: (sw, sh, dw, dh, index of the placement).  Python alone, so the share of frames outside
    the rule can be checked without a GPU."""
    rng = np.random.Generator(np.random.PCG64(0x1A4DA500 + 16 * seed + cn))
    out = []
    for _ in range(int(rng.integers(2, 25))):
        dw, dh = int(rng.integers(1, 141)), int(rng.integers(2, 13))
        while True:
            sw, sh = int(dw * rng.uniform(20.5, 62)), int(dh * rng.uniform(1.05, 40))
            if sw % dw or sh % dh:                                     # (both factors whole: resizeAreaFast_, another launch)
                break
        out.append((sw, sh, dw, dh, int(rng.integers(0, len(_places(cn))))))
    return out, rng


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_cover_fuzz(gpu, seed):
    import torch

    for cn in (1, 3):
        geoms, rng = fuzz_geometries(seed, cn)
        n = len(geoms)
        frames = [CoverFrame(torch, rng, cn, sw, sh, dw, dh, place=_places(cn)[p]) for sw, sh, dw, dh, p in geoms]
        outside = sum(not W_MIN <= widest_cell(f.sw, f.dw) <= W_MAX for f in frames)
        assert 4 * outside <= n, (outside, n)
        launches = _mixed(gpu, frames, cn)
        print("seed %d cn %d: %d frames, %d outside the rule, %d launches" % (seed, cn, n, outside, launches))
        assert 1 <= launches <= 1 + outside, (cn, n, outside, launches)
        _check_frames(gpu, frames, cn, "fuzz seed %d" % seed)


# ---------------------------------------------------------------- 4. requests through impgpu_batch_run_ops
def test_gray_requests_share_the_wide_launch(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    reqs = []
    for k in range(8):
        w, h = 1210 + 61 * k, 203 + 17 * k
        assert W_MIN <= widest_cell(w, 40) <= W_MAX and w % 40
        reqs.append(Req(noise_image(h, w, 1, 2400 + k) if k % 2 else smooth_image(h, w, 1, 110 + k), "plain", resize="40,0"))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("gray: %d requests, %d launches" % (len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert launches == 2, launches                                     # the wide launch and the promotion (before: 8 + 1)
    _release(ims, clones)
    cf.release()


def test_cropped_bgr_requests_share_the_wide_launch(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    reqs = []
    for k in range(8):
        w, h, x, y = 1210 + 61 * k, 203 + 17 * k, (1, 2, 3, 5, 6, 7, 9, 11)[k], k
        assert W_MIN <= widest_cell(w, 40) <= W_MAX and w % 40 and x % 4
        reqs.append(Req(noise_image(h + y + 2, w + x + 3, 3, 2420 + k), "plain", crop="%dpx,%dpx,%dpx,%dpx" % (w, h, x, y), resize="40,0"))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("BGR: %d cropped requests, %d launches" % (len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert launches == 1, launches                                     # (before: one table-kernel launch each, 8)
    _release(ims, clones)
    cf.release()
