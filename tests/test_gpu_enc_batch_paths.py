"""Two paths of the GIF and WebP batch encoders (impgpu_batch_encode_gif, impgpu_batch_encode_webp) that the format
tests leave out: a device failure at one entry of a batch (impgpu_fault_arm on IMP_STEP_ENCODE), and a call WITHOUT flags
that $IMPGPU_STAGE_CAP_MB cuts into groups.  The reference for a batch's entry is always its lone call: the format tests
pin the lone calls to their models."""
import numpy as np
import pytest

from test_gif_encode_host import frame_of, palette
from test_webp_writer import content

pytestmark = pytest.mark.gpu

OK, DEVICE = 0, 90
STEP_ENCODE = 8                                  # IMP_STEP_ENCODE
GIF_LAUNCHES, WEBP_LAUNCHES = 5, 6               # a group's launches without flags (include/impgpu.h)
MB = 1 << 20


def up256(n):
    return (n + 255) & ~255


def groups_under(costs, cap):
    """how many groups the encoders' rule makes: an entry that would take the running sum past the cap starts the next"""
    groups, total = 1, 0
    for c in costs:
        if total and total + c > cap:
            groups, total = groups + 1, 0
        total += c
    return groups


def gif_albums(gpu):
    rng = np.random.default_rng(77)
    sets = [[frame_of(rng, 5, 3, palette(rng, 6)) for _ in range(2)],
            [frame_of(rng, 9, 4, palette(rng, 20), transparent=0.1)],
            [frame_of(rng, 5, 3, palette(rng, 9), alpha=False) for _ in range(3)]]
    return [gpu.Image.album(frames) for frames in sets]


def webp_frames(gpu):
    return [gpu.Image(f) for f in (content("gradient_bgr", 17, 9), content("bgra_holes", 33, 18), content("noise_gray", 17, 9))]


@pytest.mark.parametrize("kind", ["gif", "webp"])
def test_a_device_failure_at_one_entry_leaves_the_others_their_lone_files(gpu, kind):
    """the n-th accepted entry enters the armed fault point: IMP_ERROR_DEVICE, length 0 and nothing written for it alone;
    the call returns IMP_OK and the other two entries, in one group's launches, are their lone calls' files"""
    images = gif_albums(gpu) if kind == "gif" else webp_frames(gpu)
    lone_call, batch_call, per_group = (gpu.encode_gif, gpu.batch_encode_gif, GIF_LAUNCHES) if kind == "gif" else \
                                       (gpu.encode_webp, gpu.batch_encode_webp, WEBP_LAUNCHES)
    lone = [lone_call(im) for im in images]
    assert all(r[0] == OK and r[3] for r in lone)
    for nth in (1, 2, 3):
        try:
            assert gpu.lib.impgpu_fault_arm(STEP_ENCODE, nth) == 0
            rc, results, launches = batch_call(images)
        finally:
            gpu.lib.impgpu_fault_arm(-1, 0)
        assert rc == OK and launches == per_group, (nth, rc, launches)
        for k, (r, want) in enumerate(zip(results, lone)):
            if k == nth - 1:
                assert r[0] == DEVICE and r[1] is None and r[2] == 0 and r[3], (nth, k, r[0], r[2], r[3])
            else:
                assert r[0] == OK and r[3] and r[1] == want[1] and r[2] == want[2], (nth, k, r[0], r[2], r[3])
    rc, results, launches = batch_call(images)                       # disarmed: the whole batch again
    assert rc == OK and launches == per_group and [r[1] for r in results] == [r[1] for r in lone]
    for im in images:
        im.release()


def test_a_flagless_gif_batch_past_the_stage_cap_goes_in_groups(gpu, monkeypatch):
    """$IMPGPU_STAGE_CAP_MB = 1: albums of 400 x 300 are counted by impgpu_gif_encode_bound (about 181 KB a frame), so
    albums of two, three and two frames sum past the cap and the third goes in a group of its own"""
    rng = np.random.default_rng(78)
    pal = palette(rng, 200)
    albums = [gpu.Image.album([frame_of(rng, 400, 300, pal[10 * k: 10 * k + 120], alpha=False) for _ in range(n)]) for k, n in enumerate((2, 3, 2))]
    lone = [gpu.encode_gif(a) for a in albums]
    assert all(r[0] == OK and r[3] for r in lone)
    costs = [gpu.gif_encode_bound(a.shape[1], a.shape[0], a.count) for a in albums]
    groups = groups_under(costs, MB)
    assert sum(costs) > MB and max(costs) <= MB and groups == 2, costs
    monkeypatch.setenv("IMPGPU_STAGE_CAP_MB", "1")
    rc, results, launches = gpu.batch_encode_gif(albums)
    monkeypatch.delenv("IMPGPU_STAGE_CAP_MB")
    print("gif groups:", costs, launches)
    assert rc == OK and launches % GIF_LAUNCHES == 0 and launches >= 2 * GIF_LAUNCHES and launches == groups * GIF_LAUNCHES, launches
    for k, (r, want) in enumerate(zip(results, lone)):
        assert r[0] == OK and r[3] and r[1] == want[1] and r[2] == want[2], k
    rc, results, launches = gpu.batch_encode_gif(albums)             # without the cap: one group
    assert rc == OK and launches == GIF_LAUNCHES and [r[1] for r in results] == [r[1] for r in lone]
    for a in albums:
        a.release()


def test_a_flagless_webp_batch_past_the_stage_cap_goes_in_groups(gpu, monkeypatch):
    """$IMPGPU_STAGE_CAP_MB = 1: a frame takes its file's bound, its residuals (4 bytes a pixel) and its work area
    (sizeof(WebpWork) = 52 224 bytes), each rounded up to 256 -- 154 112 bytes at 130 x 67 (test_gpu_webp_lz pins the same
    figure), so six fit under the cap and sixteen go in three groups"""
    names = ["gradient_bgr", "noise_gray", "bgra_holes", "noise_bgr", "two_colours", "bgra_graded", "flat_bgr", "gradient_gray"]
    frames = [content(names[k % len(names)], 130, 67) for k in range(16)]
    images = [gpu.Image(f) for f in frames]
    lone = [gpu.encode_webp(im) for im in images]
    assert all(r[0] == OK and r[3] for r in lone)
    costs = [up256(gpu.webp_encode_bound(130, 67, im.shape[2])) + up256(130 * 67 * 4) + 52224 for im in images]
    groups = groups_under(costs, MB)
    assert costs[0] == 154112 and sum(costs) > MB and groups == 3, costs
    monkeypatch.setenv("IMPGPU_STAGE_CAP_MB", "1")
    rc, results, launches = gpu.batch_encode_webp(images)
    monkeypatch.delenv("IMPGPU_STAGE_CAP_MB")
    print("webp groups:", costs[0], launches)
    assert rc == OK and launches % WEBP_LAUNCHES == 0 and launches >= 2 * WEBP_LAUNCHES and launches == groups * WEBP_LAUNCHES, launches
    for k, (r, want) in enumerate(zip(results, lone)):
        assert r[0] == OK and r[3] and r[1] == want[1] and r[2] == want[2], k
    rc, results, launches = gpu.batch_encode_webp(images)            # without the cap: one group
    assert rc == OK and launches == WEBP_LAUNCHES and [r[1] for r in results] == [r[1] for r in lone]
    for im in images:
        im.release()
