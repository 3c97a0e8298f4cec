"""impgpu_batch_run_ops with every admission class in ONE call, interleaved: requests the planner refuses (one that
impgpu_run_ops fails, one it serves) between a bare AREA shrink, a whole-factor shrink, an NN resize, a turn and an overlay on
the resize's stores, a folded overlay + flatten, a flip + blur chain, a lone blur form, gray frames with and without a resize, a
bare crop and a whole frame worked in place.

Every request must come out exactly as the per-request loop of impgpu_run_ops leaves it -- frame, code, step, and the
caller's handle where the loop keeps it -- and as the oracle chain makes it, after every fault point of steps 3 to 6 too;
the call makes the number of launches it made before its bookkeeping was gathered into one record per request."""
import numpy as np
import pytest

from conftest import noise_image, smooth_image
from test_gpu_batch_ops import Configs, Req, _pixels, check_against_loop

pytestmark = pytest.mark.gpu

# (what, channels, (width, height), frames, config, job)
KINDS = [
    ("a bare general AREA shrink", 3, (97, 61), 1, "plain", dict(resize="40,0")),
    ("refused, and failed by impgpu_run_ops: more filters than max_filters_count", 4, (83, 59), 1, "few",
     dict(crop="4,3", resize="30,0", filters=["gamma=1.1"] * 3)),
    ("a whole-factor 2x shrink", 3, (128, 96), 1, "wm", dict(resize="64,48")),
    ("refused, and served by impgpu_run_ops: a two-frame album", 3, (83, 59), 2, "wm",
     dict(crop="60px,40px,3px,2px", resize="41,0", filters=["gamma=1.2"])),
    ("a simple (NN) resize", 4, (97, 61), 1, "plain", dict(resize="50,0", simple=1)),
    ("a turn and a BGRA overlay on the resize's stores", 3, (97, 61), 1, "wm", dict(resize="44,0", filters=["rotate=90"])),
    ("overlay and flatten folded onto the resize's stores", 4, (83, 59), 1, "wm", dict(crop="4,3", resize="37,0", need_flatten=1)),
    ("a flip and a mixable blur", 3, (128, 96), 1, "plain",
     dict(crop="100px,80px,7px,5px", resize="60,0", filters=["flip=10", "blur=1.5"])),
    ("a blur whose radius is past 16: a lone form", 4, (97, 61), 1, "wm", dict(resize="48,0", filters=["blur=12"])),
    ("a gray frame with a resize", 1, (97, 61), 1, "wm", dict(resize="45,0", filters=["gamma=1.3"])),
    ("a gray frame with only a crop", 1, (83, 59), 1, "plain", dict(crop="30px,20px,3px,2px")),
    ("a bare colour crop", 3, (83, 59), 1, "plain", dict(crop="21px,13px,5px,3px")),
    ("a whole frame, pointwise: the handle stays", 4, (97, 61), 1, "wm", dict(filters=["gamma=1.4"])),
]
REFUSED_FAILED, KEEPS_HANDLE = 1, 12

# What this very call -- these requests, in this order -- launches at the commit before the batch's bookkeeping became one record
# per request (7694c0e): measured there on an MI355X with this test's body, not derived from the code under test.
LAUNCHES_AT_PARENT = 19


def _source(c, w, h, seed):
    return smooth_image(h, w, 4, seed) if c == 4 else noise_image(h, w, c, 4100 + seed)


def _requests():
    reqs = []
    for k, (_, c, (w, h), frames, cfg, job) in enumerate(KINDS):
        src = [_source(c, w, h, 10 * k + f) for f in range(frames)]
        reqs.append(Req(src if frames > 1 else src[0], cfg, **job))
    return reqs


def _configs(gpu):
    cf = Configs(gpu)
    cf.add("plain", allow_experiments=True)
    cf.add("wm", noise_image(9, 14, 4, 4050), ("r", "b", 1, 1, 70), allow_experiments=True)      # a BGRA overlay
    cf.add("few", allow_experiments=True, max_filters=2)
    return cf


_ORACLE = {}


def _oracle(cf, reqs):
    """The oracle's answer to every request, computed once for the module: [(code, step, pixels)]."""
    if not _ORACLE:
        for i, r in enumerate(reqs):
            outs = [cf.oracle(r, a) for a in (r.src if isinstance(r.src, list) else [r.src])]
            rc, step, _ = outs[-1]
            _ORACLE[i] = (rc, step, None if rc else (np.stack([o[2] for o in outs]) if isinstance(r.src, list) else outs[0][2]))
    return _ORACLE


def _check_oracle(cf, reqs, res, ims, skip=()):
    for i, (rc, step, want) in _oracle(cf, reqs).items():
        if i in skip:
            continue
        assert res[i] == (rc, step if rc else 7), (KINDS[i][0], res[i], rc, step)
        if not rc:
            got = _pixels(ims[i])
            assert got.shape == want.shape and np.array_equal(got, want), KINDS[i][0]


def _run(gpu, cf, reqs, arm=None):
    """The batch, then the loop on clones, each behind the same armed fault point.  Returns (res, launches, ims, clones, loop,
    kept, kept_loop): `kept` says per request whether the handle still has the value that went in."""
    ims = [r.image(gpu) for r in reqs]
    clones = [im.clone() for im in ims]
    before, before_loop = [im.h.value for im in ims], [cl.h.value for cl in clones]
    lib = gpu.lib
    try:
        if arm:
            assert lib.impgpu_fault_arm(*arm) == 0
        res, launches = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
        if arm:
            assert lib.impgpu_fault_arm(*arm) == 0
        loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
    finally:
        lib.impgpu_fault_arm(-1, 0)
    kept = [im.h.value == h for im, h in zip(ims, before)]
    kept_loop = [cl.h.value == h for cl, h in zip(clones, before_loop)]
    return res, launches, ims, clones, loop, kept, kept_loop


def _check_handles(reqs, ims, kept, kept_loop, step=None, target=None):
    """Which handle a request leaves with.  By impgpu_run_ops' contract it is the caller's until something writes a fresh
    frame: the two requests that write none keep it, and so does the request a fault point cuts at CROP or RESIZE, at
    FILTERING without a resize, at WATERMARK behind nothing but in-place work.  Every other request here leaves with another
    geometry than it came with -- a handle's geometry never changes, so that IS a fresh handle; its value proves nothing,
    because a request's second fresh handle can take the address its first handle was freed at."""
    for i, r in enumerate(reqs):
        keeps = i in (REFUSED_FAILED, KEEPS_HANDLE)
        if i == target:
            keeps = keeps or step in (3, 4) or (step == 5 and "resize" not in r.job)
        if keeps:
            assert kept[i] and kept_loop[i], (KINDS[i][0], step, kept[i], kept_loop[i])
        else:
            first = r.src[0] if isinstance(r.src, list) else r.src
            assert ims[i].shape != first.shape, (KINDS[i][0], step, ims[i].shape)


def _release(*groups):
    for g in groups:
        for im in g:
            im.release()


def test_every_kind_in_one_call(gpu):
    cf = _configs(gpu)
    reqs = _requests()
    res, launches, ims, clones, loop, kept, kept_loop = _run(gpu, cf, reqs)
    print("%d requests, %d launches" % (len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    _check_oracle(cf, reqs, res, ims)
    _check_handles(reqs, ims, kept, kept_loop)
    assert res[REFUSED_FAILED] == (55, 0)
    assert all(r == (0, 7) for i, r in enumerate(res) if i != REFUSED_FAILED), res
    assert all(im.shape[2] == 3 for im, kind in zip(ims, KINDS) if kind[1] == 1)      # gray comes out BGR
    assert launches == LAUNCHES_AT_PARENT, launches
    _release(ims, clones)
    cf.release()


@pytest.mark.parametrize("step", [3, 4, 5, 6])
def test_every_fault_point_cuts_the_same_request(gpu, step):
    """The nth entry into a step, for every n: the refused requests enter theirs inside impgpu_run_ops, between the planned
    requests', so any reordering of the entries makes another request fail here than in the loop."""
    cf = _configs(gpu)
    reqs = _requests()
    # who enters the step, in request order: CROP with a crop, RESIZE with a resize, FILTERING with filters or a gray frame,
    # WATERMARK with an overlay -- and nothing at all when the filter count is refused first
    entering = [i for i, (_, c, _, _, cfg, job) in enumerate(KINDS) if i != REFUSED_FAILED and
                {3: "crop" in job, 4: "resize" in job, 5: c == 1 or bool(job.get("filters")), 6: cfg == "wm"}[step]]
    assert len(entering) == {3: 5, 4: 9, 5: 7, 6: 7}[step]
    for nth, target in enumerate(entering, 1):
        res, _, ims, clones, loop, kept, kept_loop = _run(gpu, cf, reqs, arm=(step, nth))
        failed = [i for i, r in enumerate(res) if r[0] != 0 and i != REFUSED_FAILED]
        assert failed == [target], (step, nth, res)
        assert res[target] == (gpu.IMP_ERROR_DEVICE, step)
        assert res[REFUSED_FAILED] == (55, 0)
        check_against_loop(res, ims, clones, loop)
        _check_handles(reqs, ims, kept, kept_loop, step, target)
        _check_oracle(cf, reqs, res, ims, skip=failed)
        _release(ims, clones)
    cf.release()
