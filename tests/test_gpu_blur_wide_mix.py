"""impgpu_batch_run_ops: blurs of the two-pass matrix-unit form (k_blur_mfma_rows + k_blur_mfma_cols alone; blur=8 is one)
share ONE launch pair per channel count and byte-plane count, through k_blur_rows_mix + k_blur_cols_mix.

Every request must come out exactly as the per-request loop of impgpu_run_ops leaves it -- frame, code, step -- and as the
oracle chain makes it (its Gaussian is exact).  Launch counts are measured against calls made in the same process.

Before the shared launch pair existed every such blur took its own two launches; the counts this file's calls made then,
measured on an MI355X with this file: PARENT_LAUNCHES below."""
import numpy as np
import pytest

from conftest import noise_image, smooth_image
from test_gpu_batch_ops import Configs, Req, check_against_loop, check_against_oracle, run_both

pytestmark = pytest.mark.gpu

# Sigmas of the two-pass matrix-unit form (impgpu_blur_form == 3) for BGR and BGRA alike, found with impgpu_blur_form's sweep
# over 0.5 .. 25.0 in steps of 0.1 (tests/test_blur_form.py checks them on the host): two byte planes at sigma 8 -- as at every
# two-pass sigma but a few -- and three planes (tap sums of 258 .. 260) at 7.7, 7.9 and 10.5 for both channel counts (BGR
# also 7.4, 7.5; BGRA also 6.5, 7.3, 7.4, 7.5).  7.7 and 10.5 differ in radius.
SIGMA_PAIR_2 = 8.0
SIGMAS_PAIR_3 = (7.7, 10.5)
SIGMAS_PAIR_2_MORE = (12.0, 18.0)        # two planes too, larger radii (more 64-byte chunks per window)
SIGMAS_ONE_PASS = (2.0, 1.5)             # k_blur_mfma_fused with two planes (impgpu_blur_form == 2): the chains' control
# What the calls of the first four tests launched before the launch pair was shared (this file against the parent commit's
# library on an MI355X; with the shared pair: 10, 8, 8 and 14), so the four fail there on their launch counts.
PARENT_LAUNCHES = {"shared": 22, "shapes": 38, "windows": 24, "chains": 46}


def _src(c, w, h, seed):
    return noise_image(h, w, 3, 5200 + seed) if c == 3 else smooth_image(h, w, 4, seed)


def _plain(gpu):
    cf = Configs(gpu)
    cf.add("plain", allow_experiments=True)
    cf.add("wm", noise_image(9, 14, 4, 5290), ("r", "b", 1, 1, 70), allow_experiments=True)
    return cf


def _release(*groups):
    for g in groups:
        for im in g or ():
            im.release()


def _launches(gpu, cf, reqs):
    """What a call launches, its frames not looked at."""
    _, launches, ims, _, _ = run_both(gpu, cf, reqs, compare_loop=False)
    _release(ims)
    return launches


def _checked(gpu, cf, reqs):
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert all(r == (0, 7) for r in res), res
    _release(ims, clones)
    return launches


def _without_blur(reqs):
    out = []
    for r in reqs:
        job = dict(r.job)
        job["filters"] = [f for f in job.get("filters", ()) if not f.startswith("blur=")]
        out.append(Req(r.src, r.cfg, **job))
    return out


def _resized(c, k, sigma, **more):
    """A resized request of its own geometry: a general AREA shrink (no whole factor), so all of them share one resize launch
    per channel count."""
    w, h = 200 - 7 * k, 150 - 5 * k
    return Req(_src(c, w, h, 10 * k + c), "plain", resize="%d,0" % (97 - 6 * k), filters=["blur=%g" % sigma], **more)


def test_wide_blurs_share_two_launches_per_class(gpu):
    cf = _plain(gpu)
    reqs = []
    for c in (3, 4):
        reqs += [_resized(c, k, SIGMA_PAIR_2) for k in range(3)]
        reqs += [_resized(c, 3 + k, SIGMAS_PAIR_3[k]) for k in range(2)]
    assert len({(r.src.shape, r.job["resize"]) for r in reqs}) == len(reqs)
    base = _launches(gpu, cf, _without_blur(reqs))
    launches = _checked(gpu, cf, reqs)
    print("bare resizes %d launches, with the blurs %d (one launch pair each: %d)" % (base, launches, base + 2 * len(reqs)))
    assert base == 2                                      # one general AREA launch per channel count
    assert launches == base + 2 * 4, launches             # (BGR, BGRA) x (two planes, three planes)
    cf.release()


# (channels, width, height, sigma): whole frames without a resize, so the blur runs on exactly these shapes
SHAPES = [
    (3, 48, 30, 18.0), (4, 48, 30, 18.0),        # smaller than one tile, the radius past the frame: borders replicate on every side
    (3, 48, 30, 8.0), (4, 48, 30, 8.0),
    (3, 65, 65, 8.0), (4, 65, 65, 8.0),          # one row and one pixel column into a second tile
    (3, 43, 65, 8.0),                            # 129 bytes across: ONE byte into a third tile
    (3, 61, 47, 8.0),                            # (w * 3) & 3 == 3: the last bytes of a row take OpenCV's scalar rounding
    (3, 62, 64, 12.0),                           # (w * 3) & 3 == 2, another radius
    (3, 64, 50, 8.0),                            # (w * 3) % 64 == 0
    (4, 80, 64, 8.0), (3, 70, 128, 12.0), (4, 33, 128, 12.0),      # heights that are multiples of 64; two radii per class
    (3, 150, 97, 7.7), (3, 61, 64, 10.5), (4, 149, 90, 7.7), (4, 64, 65, 10.5),     # three planes, two radii per class
    (3, 200, 150, 8.0), (4, 200, 150, 18.0),
]


def test_shapes_where_a_tile_body_can_go_wrong(gpu):
    cf = _plain(gpu)
    reqs = [Req(_src(c, w, h, 100 + k), "plain", filters=["blur=%g" % s]) for k, (c, w, h, s) in enumerate(SHAPES)]
    assert {s for _, _, _, s in SHAPES} <= {SIGMA_PAIR_2, *SIGMAS_PAIR_2_MORE, *SIGMAS_PAIR_3}
    launches = _checked(gpu, cf, reqs)
    print("%d whole frames, %d launches (one pair each: %d)" % (len(reqs), launches, 2 * len(reqs)))
    assert launches == 2 * 4, launches                    # nothing but the four classes' launch pairs
    cf.release()


def _windowed(c, sigma=SIGMA_PAIR_2):
    """Requests without a resize whose blur reads a crop window: BGR windows that start at byte addresses off the dword grid
    (column 3, 5 and 7 of a 3-channel row: byte 9, 15, 21), BGRA windows (always on it)."""
    return [Req(_src(c, 180, 140, 200 + c), "plain", crop="120px,90px,3px,2px", filters=["blur=%g" % sigma]),
            Req(_src(c, 171, 133, 210 + c), "plain", crop="97px,101px,5px,7px", filters=["blur=%g" % sigma]),
            Req(_src(c, 200, 150, 220 + c), "plain", crop="64px,64px,7px,1px", filters=["blur=%g" % sigma, "gamma=1.3"])]


def test_windows_join_the_resized_requests_launch_pair(gpu):
    cf = _plain(gpu)
    resized = [_resized(c, k, SIGMA_PAIR_2) for c in (3, 4) for k in range(2)]
    windows = _windowed(3) + _windowed(4)
    base = _launches(gpu, cf, _without_blur(resized))
    tail = 2                                              # the gamma behind two of the windows' blurs: one launch per channel count
    launches = _checked(gpu, cf, resized + windows)
    print("resizes %d launches, with %d resized and %d windowed blurs %d" % (base, len(resized), len(windows), launches))
    assert launches == base + 2 * 2 + tail, launches
    # The caller's frames: the windowed requests' sources as caller-owned buffers (wrapped, so they outlive their handles),
    # served in the same launch pairs as the resized requests.  k_blur_rows_mix must only read them: afterwards every buffer
    # is its source array byte for byte, outside and inside the window.
    import torch

    reqs = resized + windows
    bufs = [torch.from_numpy(r.src.copy()).cuda() for r in windows]
    torch.cuda.synchronize()
    ims = [r.image(gpu) for r in resized]
    ims += [gpu.Image.wrap(b.data_ptr(), r.src.shape[1], r.src.shape[0], r.src.shape[2], r.src.shape[1] * r.src.shape[2])
            for b, r in zip(bufs, windows)]
    res, wrapped_launches = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
    assert all(r == (0, 7) for r in res), res
    assert wrapped_launches == launches                   # the same pairs: the windows joined the resized requests'
    check_against_oracle(cf, reqs, res, ims)
    gpu.sync()
    for b, r in zip(bufs, windows):
        assert np.array_equal(b.cpu().numpy(), r.src), r.job
    _release(ims)
    # ... and a request cut at FILTERING keeps its frame, uncropped, while the other windows are read in the same launch pair.
    for target in (len(resized), len(resized) + 3):
        nth = 1 + target                                  # every request here enters FILTERING, in request order
        ims = [r.image(gpu) for r in reqs]
        try:
            assert gpu.lib.impgpu_fault_arm(5, nth) == 0
            res, _ = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
        finally:
            gpu.lib.impgpu_fault_arm(-1, 0)
        assert [i for i, r in enumerate(res) if r[0]] == [target] and res[target] == (gpu.IMP_ERROR_DEVICE, 5), res
        assert np.array_equal(ims[target].numpy(), reqs[target].src)
        check_against_oracle(cf, reqs, res, ims, skip=(target,))
        _release(ims)
    cf.release()


def _chains(sigma_a, sigma_b):
    """Per channel count and twice each, on different geometry: a wide blur then a pointwise filter; a flip, then the blur; the
    blur as the last segment with the overlay (and for BGRA the flatten) behind it; two wide blurs in one chain."""
    reqs = []
    for c in (3, 4):
        for k in range(2):
            flat = dict(need_flatten=1) if c == 4 else {}
            reqs += [_resized(c, 4 * k, sigma_a),
                     _resized(c, 4 * k + 1, sigma_a),
                     _resized(c, 4 * k + 2, sigma_a, **flat),
                     _resized(c, 4 * k + 3, sigma_a)]
            reqs[-4].job["filters"] = ["blur=%g" % sigma_a, "gamma=1.3"]
            reqs[-3].job["filters"] = ["flip=10", "blur=%g" % sigma_a]
            reqs[-2].cfg = "wm"
            reqs[-1].job["filters"] = ["blur=%g" % sigma_a, "blur=%g" % sigma_b]
    return reqs


def test_chains_with_wide_blurs(gpu):
    """The same chains with one-pass sigmas in the blurs' places make the same rounds with ONE launch per blur class; the wide
    blurs make two.  Round 1 (the segments behind the resize) blurs three chains per channel count, round 2 two: four
    classes."""
    cf = _plain(gpu)
    base = _launches(gpu, cf, _chains(*SIGMAS_ONE_PASS))
    launches = _checked(gpu, cf, _chains(SIGMA_PAIR_2, SIGMAS_PAIR_2_MORE[0]))
    print("one-pass blurs %d launches, wide blurs %d" % (base, launches))
    assert launches == base + 4, (launches, base)
    cf.release()


def test_every_fault_point_cuts_the_same_request(gpu):
    """FILTERING armed for the nth entry, every n of a six-request call.  Cutting one of the two BGRA requests leaves the other
    a class of one (the lone path); cutting a BGR request leaves three that still share."""
    cf = _plain(gpu)
    reqs = [_resized(3, 0, SIGMA_PAIR_2), _resized(4, 1, SIGMA_PAIR_2), _windowed(3)[1], _resized(4, 2, SIGMA_PAIR_2),
            _resized(3, 3, SIGMA_PAIR_2), _windowed(3)[2]]
    want = [cf.oracle(r, r.src) for r in reqs]
    for nth in range(1, len(reqs) + 1):
        target = nth - 1
        ims = [r.image(gpu) for r in reqs]
        clones = [im.clone() for im in ims]
        try:
            assert gpu.lib.impgpu_fault_arm(5, nth) == 0
            res, _ = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
            assert gpu.lib.impgpu_fault_arm(5, nth) == 0
            loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
        finally:
            gpu.lib.impgpu_fault_arm(-1, 0)
        assert [i for i, r in enumerate(res) if r[0]] == [target], (nth, res)
        assert res[target] == (gpu.IMP_ERROR_DEVICE, 5)
        check_against_loop(res, ims, clones, loop)
        for i, (rc, _, px) in enumerate(want):
            if i != target:
                assert res[i] == (0, 7) and np.array_equal(ims[i].numpy(), px), (nth, i)
        _release(ims, clones)
    cf.release()


def test_a_class_of_one_keeps_the_lone_path(gpu):
    """One wide blur among bare resizes: two launches more than the resizes, as before the launch pair was shared.  The count
    alone cannot tell the lone kernels from a launch pair over one descriptor (both are two launches); that a class of one
    goes through apply_plan is Batch::segment_round's `cls.size() == 1` branch, known by reading."""
    cf = _plain(gpu)
    reqs = [Req(_src(c, 200 - 9 * k, 150 - 4 * k, 300 + k), "plain", resize="%d,0" % (91 - 5 * k)) for k, c in enumerate((3, 4, 3, 4, 3))]
    reqs.insert(2, _resized(4, 5, SIGMA_PAIR_2))
    base = _launches(gpu, cf, _without_blur(reqs))
    launches = _checked(gpu, cf, reqs)
    assert launches == base + 2, (launches, base)
    cf.release()
