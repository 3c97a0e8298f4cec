"""Requests WITHOUT a resize on the batched path: a crop's window leaves its frame through ONE window launch per channel count
(k_window_mix: the bare crop as 16-byte runs, or the chain's first pointwise segment / watermark / flatten read from the
window), a gray window through the call's single promotion, a flip / turn / one-pass blur with the window as its source.

Every request must come out exactly as the per-request loop of impgpu_run_ops leaves it -- frame, code, step, after a fault
point too -- and as the oracle chain makes it; the number of kernels enqueued must not depend on the number of requests."""
import numpy as np
import pytest

from conftest import noise_image, smooth_image
from test_gpu_batch_ops import Configs, Req, check_against_loop, check_against_oracle, run_both

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PARENTS = [(37, 29), (64, 48)]                                  # (width, height)
WIDTHS = [1, 5, 6, 16, 17, 21, 22]                              # BGR row bytes 3, 15, 18, 48, 51, 63, 66: around the 16-byte run
HEIGHTS = [1, 2, 7]


def _crop(w, h, x, y):
    return "%dpx,%dpx,%dpx,%dpx" % (w, h, x, y)


def _windows(pw, ph, widths=WIDTHS, heights=HEIGHTS):
    """(w, h, x, y): every x in 0..4 (BGR byte offsets 0, 3, 2, 1, 0 mod 4) with every width and height, windows that touch
    the right and the bottom edge, the bottom right corner, and the whole frame."""
    out = []
    for x in range(5):
        for w in widths:
            for h in heights:
                out.append((w, h, x, (x + w + h) % 5))
    for w in widths:
        out.append((w, heights[-1], pw - w, 1))                 # right edge
        out.append((w, heights[-1], 2, ph - heights[-1]))       # bottom edge
        out.append((w, heights[1], pw - w, ph - heights[1]))    # the corner: the frame's last byte
    out.append((pw, ph, 0, 0))
    return out


def _parent(pw, ph, c, seed):
    return noise_image(ph, pw, c, 3000 + seed) if c != 4 else smooth_image(ph, pw, 4, seed)


def _configs(gpu):
    cf = Configs(gpu)
    cf.add("plain", allow_experiments=True)
    cf.add("wm", noise_image(9, 14, 4, 3050), ("r", "b", 1, 1, 70), allow_experiments=True)      # a BGRA overlay
    cf.add("hang", noise_image(12, 30, 3, 3051), ("r", "b", -4, -3, 45), allow_experiments=True)  # BGR, hanging over the edge
    return cf


def _release(*groups):
    for g in groups:
        for im in g or ():
            im.release()


def _raw(gpu, im, extra=0):
    """The frame's memory as the device holds it -- every row with its pitch padding, and `extra` bytes behind the last row."""
    h, _, _ = im.shape
    n = im.step * h + extra
    view = gpu.Image.wrap(im.device_ptr, n, 1, 1, n)
    out = view.numpy().reshape(-1)
    view.release()
    return out


_HELD = []


def _colour_the_pool(gpu, drain=8192, give=1024):
    """Leave the front of the pool's smallest bucket (4 KiB: where every frame of these tests lives) filled with CANARY.  The
    pool hands out a bucket's free blocks oldest first, so the stale ones have to go: `drain` frames are created at once --
    more than the bucket's free list holds -- and written with the canary; `give` of them go back, the rest stay out of
    circulation until the module ends.  The frames the next call creates are then known byte for byte before anything is
    stored to them.

    This leans on the pool as imp_runtime.hip has it: bucket_of() puts everything up to 4 KiB into one bucket, dev_alloc takes
    the first block of a bucket's std::multimap range and lane_take_back appends behind the last (oldest first),
    image_new_album asks for 16 bytes more than the frame, and a session never has 8192 free blocks of that bucket.  A pool
    with another policy needs another way to colour fresh frames here; the assertions that depend on it are the two CANARY
    ones of test_bare_crops_every_alignment, which can fail for that reason but cannot let a stray store pass."""
    fill = np.full((1, 4080, 1), CANARY, dtype=np.uint8)       # 4080 + the 16 bytes every frame's block has behind it
    held = [gpu.Image(fill) for _ in range(drain)]
    gpu.sync()
    _release(held[:give])
    _HELD.extend(held[give:])


@pytest.fixture(scope="module", autouse=True)
def _hand_the_pool_back():
    yield
    _release(_HELD)
    del _HELD[:]


# ---------------------------------------------------------------- 1. the bare crop, every alignment
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("parent", range(len(PARENTS)))
def test_bare_crops_every_alignment(gpu, parent, c):
    pw, ph = PARENTS[parent]
    cf = _configs(gpu)
    a = _parent(pw, ph, c, 10 * parent + c)
    wins = _windows(pw, ph)
    reqs = [Req(a, "plain", crop=_crop(*win)) for win in wins]
    ims = [r.image(gpu) for r in reqs]
    clones = [im.clone() for im in ims]
    handles = [im.h.value for im in ims]
    _colour_the_pool(gpu)
    res, launches = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
    # what the call stored, with the memory around it: rows' padding and the 16 bytes behind the frame still hold the canary
    for im, (w, h, x, y) in zip(ims[:-1], wins[:-1]):
        raw = _raw(gpu, im, 16)
        rows = raw[:im.step * h].reshape(h, im.step)
        assert np.array_equal(rows[:, :w * c].reshape(h, w, c), a[y:y + h, x:x + w]), (w, h, x, y)
        assert (rows[:, w * c:] == CANARY).all(), ("pitch padding", w, h, x, y)
        assert (raw[im.step * h:] == CANARY).all(), ("behind the frame", w, h, x, y)
    loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert all(r == (0, 7) for r in res)
    assert ims[-1].h.value == handles[-1]                      # the whole frame: nothing to copy, the handle stays
    assert all(im.h.value != hd for im, hd in zip(ims[:-1], handles[:-1]))
    assert launches == 1, launches
    _release(ims, clones)
    cf.release()


def test_bare_crops_of_a_wrapped_frame_with_an_odd_pitch(gpu):
    """A caller's buffer of exactly 37 x 29 BGR pixels at a pitch of 111 bytes: rows start at every byte alignment and nothing
    lies behind the last one, so the windows that touch the last row and column are where a wide load could leave the buffer.
    What this checks on the device is the bytes copied and that the caller's buffers are only read; a load past the buffer's
    end would land in the allocator's slack and go unseen here -- that no load leaves a window row is checked on the host,
    under AddressSanitizer, by tools/copy_run_host_check.py."""
    import torch

    pw, ph = PARENTS[0]
    cf = _configs(gpu)
    a = _parent(pw, ph, 3, 77)
    wins = _windows(pw, ph)[:-1] + [(pw, 1, 0, ph - 1), (1, ph, pw - 1, 0), (pw - 1, ph - 1, 1, 1)]
    bufs = [torch.from_numpy(a.copy()).cuda() for _ in wins]
    torch.cuda.synchronize()
    ims = [gpu.Image.wrap(b.data_ptr(), pw, ph, 3, pw * 3) for b in bufs]
    jobs = [dict(crop=_crop(*win)) for win in wins]
    res, launches = gpu.batch_run_ops(ims, [cf.cfg["plain"]] * len(ims), jobs)
    assert launches == 1, launches
    for im, r, (w, h, x, y) in zip(ims, res, wins):
        assert r == (0, 7)
        assert np.array_equal(im.numpy(), a[y:y + h, x:x + w]), (w, h, x, y)
    gpu.sync()
    for b in bufs:
        assert np.array_equal(b.cpu().numpy(), a)              # the caller's frames are only read
    _release(ims)
    cf.release()


# ---------------------------------------------------------------- 2. the same windows with filters, overlays, flatten
FILTERS = [["gamma=1.4"], ["vignette=0.8,0.6"], ["flip=10"], ["rotate=90"], ["blur=1.5"], ["gamma=1.2", "blur=1", "contrast=1.3"]]


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("filters", range(len(FILTERS)))
def test_filtered_windows_match_loop_and_oracle(gpu, filters, c):
    cf = _configs(gpu)
    reqs = []
    for p, (pw, ph) in enumerate(PARENTS):
        a = _parent(pw, ph, c, 20 * p + c)
        for k, win in enumerate(_windows(pw, ph)):                     # the windows of the bare crops, all of them
            cfg = ("plain", "wm", "hang")[(k + k // 3) % 3]            # (every height meets every config)
            reqs.append(Req(a, cfg, crop=_crop(*win), filters=FILTERS[filters], need_flatten=int(c == 4 and k % 2 == 0)))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("%s, %d channels: %d requests, %d launches" % (FILTERS[filters], c, len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    _release(ims, clones)
    cf.release()


@pytest.mark.parametrize("c", [3, 4])
def test_watermark_and_flatten_alone_on_windows(gpu, c):
    cf = _configs(gpu)
    reqs = []
    for p, (pw, ph) in enumerate(PARENTS):
        a = _parent(pw, ph, c, 40 * p + c)
        # (proper windows only: a whole frame runs in place, in the round's k_pixel_tail_mix group -- test_whole_frames_stay_in_place)
        # -- and a window of one row or one column has no room for the "wm" overlay: that request is refused at the watermark
        # step by impgpu_run_ops inside the call, before anything is launched)
        for k, win in enumerate(_windows(pw, ph)[:-1]):
            reqs.append(Req(a, ("wm", "hang", "plain")[(k + k // 3) % 3], crop=_crop(*win), need_flatten=int(c == 4)))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert launches == 1, launches                             # overlays, flattens and bare crops: items of one launch
    _release(ims, clones)
    cf.release()


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("c", [3, 4])
def test_windows_a_blur_leaves_in_place_are_copied_out_once(gpu, n, c):
    """One-row and one-column windows: no one-pass blur form takes them, so the blur works in place on the window, two
    launches per request (rows, columns) as in impgpu_run_ops -- and the windows then leave in ONE window launch behind the
    last round, whatever their number.  A 1 x 1 window is not blurred at all and is copied out by the same launch."""
    cf = _configs(gpu)
    a = _parent(64, 48, c, 50 + c)
    reqs = []
    for k in range(n):
        w, h = (1, 5 + k) if k % 2 else (6 + k, 1)
        reqs.append(Req(a, "plain", crop=_crop(w, h, 1 + k, 2 + k), filters=["blur=1.5"]))
    reqs.append(Req(a, "plain", crop=_crop(1, 1, 3, 3), filters=["blur=1.5"]))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert all(r == (0, 7) for r in res)
    assert launches == 2 * n + 1, (n, launches)
    _release(ims, clones)
    cf.release()


# ---------------------------------------------------------------- 3. gray
def test_gray_windows_come_out_bgr(gpu):
    cf = _configs(gpu)
    reqs = []
    for k in range(12):
        a = noise_image(21, 33, 1, 3200 + k)
        win = _crop(5 + k, 3 + k % 7, k % 5, k % 4)
        reqs.append(Req(a, "plain", crop=win))
        reqs.append(Req(a, "plain", crop=win, filters=["gamma=1.4"]))
        reqs.append(Req(a, ("wm", "hang")[k % 2]))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert all(im.shape[2] == 3 for im in ims)
    assert launches == 2, launches                             # the promotion, and the tail (gamma; the overlays) in place
    _release(ims, clones)
    cf.release()


# ---------------------------------------------------------------- 4. no crop, no resize
@pytest.mark.parametrize("c", [3, 4])
def test_whole_frames_stay_in_place(gpu, c):
    cf = _configs(gpu)
    a = _parent(64, 48, c, 60 + c)
    for cfg, job, expect in [("plain", dict(filters=["gamma=1.4", "contrast=1.2"]), 1),
                             ("wm", dict(), 1),
                             ("plain", dict(need_flatten=1), 1 if c == 4 else 0),
                             ("plain", dict(), 0),
                             ("plain", dict(crop=_crop(64, 48, 0, 0)), 0)]:
        reqs = [Req(a, cfg, **job) for _ in range(4)]
        ims = [r.image(gpu) for r in reqs]
        clones = [im.clone() for im in ims]
        handles = [im.h.value for im in ims]
        res, launches = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
        loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
        check_against_loop(res, ims, clones, loop)
        check_against_oracle(cf, reqs, res, ims)
        assert [im.h.value for im in ims] == handles, (cfg, job)
        assert launches == expect, (cfg, job, launches)
        _release(ims, clones)
    cf.release()


# ---------------------------------------------------------------- 5. launch counts: the same for 4 and for 32 requests
def _spread(n, c, seed):
    """n sources of n sizes with n different windows, x offsets 0..3 all present."""
    out = []
    for k in range(n):
        pw, ph = 40 + 7 * k, 30 + 5 * k
        out.append((_parent(pw, ph, c, seed + k), _crop(9 + 3 * k, 5 + 2 * k, k % 4 + (k // 4) % 3, k % 6)))
    return out


def _count(gpu, cf, reqs):
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert all(r == (0, 7) for r in res)
    _release(ims, clones)
    return launches


@pytest.mark.parametrize("n", [4, 32])
def test_launch_counts(gpu, n):
    """On the per-request path each of these requests cost one to three launches of its own."""
    cf = _configs(gpu)
    bgr = [Req(a, "plain", crop=win) for a, win in _spread(n, 3, 100)]
    assert _count(gpu, cf, bgr) == 1
    both = [Req(a, "plain", crop=win) for a, win in _spread(n // 2, 3, 200) + _spread(n // 2, 4, 300)]
    assert _count(gpu, cf, both) == 2
    chain = [Req(a, "wm", crop=win, filters=["gamma=1.3"]) for a, win in _spread(n, 3, 400)]
    assert _count(gpu, cf, chain) == 1
    gray = [Req(a, "plain", crop=win) for a, win in _spread(n, 1, 500)]
    assert _count(gpu, cf, gray) == 1
    cf.release()


@pytest.mark.parametrize("n", [4, 16, 32])
def test_gray_crops_share_the_promotion(gpu, n):
    cf = _configs(gpu)
    assert _count(gpu, cf, [Req(a, "plain", crop=win) for a, win in _spread(n, 1, 600)]) == 1
    cf.release()


@pytest.mark.parametrize("n", [4, 32])
def test_mixed_call_meets_the_launch_bound(gpu, n):
    """Requests without a resize next to resized ones: they add the window launches -- at most two per colour channel count --
    and nothing else; their promotion and their later rounds are the launches the resized requests make anyway."""
    cf = _configs(gpu)
    sized = []
    for k in range(4):
        h, w = 203 + 31 * k, 301 + 47 * k
        sized.append(Req(noise_image(h, w, 3, 3300 + k), "plain", resize="120,0", filters=["gamma=1.2"]))
        sized.append(Req(smooth_image(h, w, 4, k), "plain", resize="120,0", filters=["gamma=1.2"]))
        sized.append(Req(noise_image(h, w, 1, 3310 + k), "wm", resize="120,0", filters=["gamma=1.2"]))
    alone = _count(gpu, cf, sized)
    unsized = []
    for k, ((a3, w3), (a4, w4), (a1, w1)) in enumerate(zip(_spread(n, 3, 700), _spread(n, 4, 800), _spread(n, 1, 900))):
        unsized.append(Req(a3, "plain", crop=w3))                                      # bare crops
        unsized.append(Req(a4, "plain", crop=w4))
        unsized.append(Req(a3, "wm", crop=w3, filters=["gamma=1.3"]))                  # crop + gamma + watermark
        unsized.append(Req(a4, "hang", crop=w4, filters=["vignette=0.8,0.6"], need_flatten=1))
        unsized.append(Req(a1, "plain", crop=w1))                                      # gray
        unsized.append(Req(a1, "wm", crop=w1, filters=["gamma=1.3"]))
    mixed = [r for pair in zip(unsized, (sized * len(unsized))[:len(unsized)]) for r in pair]
    with_unsized = _count(gpu, cf, mixed)
    print("n = %d: %d resized requests alone: %d launches; with %d requests without a resize: %d" %
          (n, len(sized), alone, len(unsized), with_unsized))
    # BGR: one window launch (bare + gamma/overlay items); BGRA: two (bare, and the vignette group)
    assert with_unsized - alone <= 2 * 2
    assert with_unsized - alone == 3, (alone, with_unsized)
    cf.release()


# ---------------------------------------------------------------- 6. fault points
# (channels, config, job)
FAULT_REQS = [(3, "plain", dict(crop=_crop(21, 7, 1, 2))),
              (3, "wm", dict(crop=_crop(22, 9, 2, 1), filters=["gamma=1.3"])),
              (4, "wm", dict(crop=_crop(17, 8, 3, 3), filters=["gamma=1.3"], need_flatten=1)),
              (3, "wm", dict(crop=_crop(19, 11, 3, 0), filters=["rotate=90"])),
              (1, "plain", dict(crop=_crop(15, 6, 1, 1), filters=["gamma=1.3"])),
              (3, "plain", dict(filters=["gamma=1.3"])),
              (3, "wm", dict(crop=_crop(16, 5, 5, 4))),
              (1, "wm", dict(crop=_crop(13, 9, 2, 2), filters=["gamma=1.3"])),
              (4, "hang", dict(filters=["gamma=1.3"]))]


@pytest.mark.parametrize("step", [3, 5, 6])
def test_fault_points_cut_the_same_request(gpu, step):
    cf = _configs(gpu)
    reqs = [Req(_parent(37, 29, c, 70 + k), cfg, **job) for k, (c, cfg, job) in enumerate(FAULT_REQS)]
    # the requests that enter the step, in order: CROP with a crop; FILTERING with filters or a gray frame; WATERMARK with an
    # overlay.  None of them enters RESIZE.
    entering = [i for i, (c, cfg, job) in enumerate(FAULT_REQS)
                if (step != 3 or "crop" in job) and (step != 5 or c == 1 or job.get("filters")) and (step != 6 or cfg != "plain")]
    lib = gpu.lib
    for nth, target in enumerate(entering, 1):
        ims = [r.image(gpu) for r in reqs]
        clones = [im.clone() for im in ims]
        handles = [im.h.value for im in ims]
        try:
            assert lib.impgpu_fault_arm(step, nth) == 0
            res, _ = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
            assert lib.impgpu_fault_arm(step, nth) == 0
            loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
        finally:
            lib.impgpu_fault_arm(-1, 0)
        failed = [i for i, r in enumerate(res) if r[0] != 0]
        assert failed == [target], (step, nth, res)
        assert res[target] == (gpu.IMP_ERROR_DEVICE, step)
        check_against_loop(res, ims, clones, loop)
        check_against_oracle(cf, reqs, res, ims, skip=failed)
        c, cfg, job = FAULT_REQS[target]
        got = ims[target].numpy()
        src = reqs[target].src
        if step in (3, 5):                                     # nothing was written: the uncropped frame, the handle itself
            assert ims[target].h.value == handles[target]
            assert np.array_equal(got, src)
        elif c != 1 and job.get("filters") == ["gamma=1.3"] and "crop" in job:
            # cut at WATERMARK behind a pointwise run on a window: the uncropped frame, filtered inside the window only
            assert ims[target].h.value == handles[target]
            w, h, x, y = (int(v[:-2]) for v in job["crop"].split(","))
            rc, _, want = cf.oracle(Req(src, "plain", crop=job["crop"], filters=job["filters"]), src)
            assert rc == 0 and np.array_equal(got[y:y + h, x:x + w], want)
            outside = np.ones(src.shape[:2], dtype=bool)
            outside[y:y + h, x:x + w] = False
            assert np.array_equal(got[outside], src[outside])
        _release(ims, clones)
    cf.release()


# ---------------------------------------------------------------- 7. the lone path
@pytest.mark.parametrize("c", [1, 3, 4])
def test_lone_crop_and_clone_equal_slicing(gpu, c):
    import torch

    pw, ph = PARENTS[0]
    a = _parent(pw, ph, c, 90 + c)
    for w, h, x, y in _windows(pw, ph):
        im = gpu.Image(a)
        assert im.crop(_crop(w, h, x, y)) == 0
        assert np.array_equal(im.numpy(), a[y:y + h, x:x + w]), (w, h, x, y)
        twin = im.clone()
        assert np.array_equal(twin.numpy(), a[y:y + h, x:x + w]), (w, h, x, y)
        _release([im, twin])
    # a caller's buffer at a pitch that is no multiple of 4: the clone of the whole frame, and crops that touch its last byte
    buf = torch.from_numpy(a.copy()).cuda()
    torch.cuda.synchronize()
    for w, h, x, y in [(pw, ph, 0, 0), (pw - 1, ph - 1, 1, 1), (22, 7, pw - 22, ph - 7), (pw, 1, 0, ph - 1)]:
        im = gpu.Image.wrap(buf.data_ptr(), pw, ph, c, pw * c)
        twin = im.clone()
        assert np.array_equal(twin.numpy(), a)
        assert im.crop(_crop(w, h, x, y)) == 0
        assert np.array_equal(im.numpy(), a[y:y + h, x:x + w]), (w, h, x, y)
        _release([im, twin])
    gpu.sync()
    assert np.array_equal(buf.cpu().numpy(), a)
