"""impgpu_batch_calc_perceived_brightness / impgpu_batch_ascii: the json and text exits (Info(), bridge.c:283-300;
ASCII(), filters.c:486-522) of many frames in one call.  Every value, text and frame must be what the lone call gives
for that frame alone -- which is what the CPU oracle gives -- bit for bit; the number of launches follows the channel
counts present, not the number of frames."""
import threading

import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image, smooth_image

pytestmark = pytest.mark.gpu

INVALID, DEVICE = 50, 90            # IMP_ERROR_INVALID_ARGS, IMP_ERROR_DEVICE
STEP_INFO = 7


# ---- contents (the recipes of test_brightness_adversarial_exact, for any geometry and channel count) ----
def _noise(rng, h, w, c):
    return rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)


def _flat100(rng, h, w, c):
    """The frame whose float accumulator stalls (test_brightness_float_accumulator_is_not_the_true_mean)."""
    return np.full((h, w, c), 100, np.uint8)


def _gray_equal(rng, h, w, c):
    """B = G = R: every term is an integer, so every addition that can tie does."""
    g = rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8)
    if c == 1:
        return g
    a = g.repeat(3, axis=2)
    return a if c == 3 else np.concatenate([a, rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8)], axis=2)


def _zero_prefix(rng, h, w, c):
    """The walk visits columns first: two thirds of the columns black, then noise."""
    a = np.zeros((h, w, c), np.uint8)
    k = (2 * w) // 3
    a[:, k:] = rng.integers(0, 256, size=(h, w - k, c), dtype=np.uint8)
    return a


def _white(rng, h, w, c):
    return np.full((h, w, c), 255, np.uint8)


def _dark_then_bright(rng, h, w, c):
    a = rng.integers(0, 2, size=(h, w, c), dtype=np.uint8)
    a[:, w // 2:] = rng.integers(200, 256, size=(h, w - w // 2, c), dtype=np.uint8)
    return a


CONTENTS = [_noise, _flat100, _gray_equal, _zero_prefix, _white, _dark_then_bright]
# (width, height): 64 x 64 has no summaries (ne = 0), 257 x 16 = 4112 pixels is the last size without, 3 x 1371 = 4113 the first with one binade
SMALL = [(1, 1), (3, 5), (64, 64), (257, 16), (3, 1371), (224, 224), (300, 256), (640, 480)]


def mixed_pool():
    rng = np.random.Generator(np.random.PCG64(0x1F0B))
    frames = []
    k = 0
    for (w, h) in SMALL:
        for c in (1, 3, 4):
            frames.append(CONTENTS[k % len(CONTENTS)](rng, h, w, c))
            k += 1
    for k, make in enumerate(CONTENTS):
        frames.append(make(rng, 480, 640, 3))
        frames.append(make(rng, 256, 300, 4))
        frames.append(make(rng, 1080, 1920, (3, 3, 4, 3, 1, 3)[k]))
    frames.append(_noise(rng, 2160, 3840, 4))
    return frames


def f32(x):
    return np.float32(x)


def lone_values(gpu, ims):
    """The lone call on a clone of every frame (the second witness)."""
    out = []
    for im in ims:
        cl = im.clone()
        out.append(cl.calc_perceived_brightness())
        cl.release()
    return out


def release(*lists):
    for ims in lists:
        for im in ims:
            if im is not None:
                im.release()


def test_mixed_pool_brightness(gpu):
    frames = mixed_pool()
    assert len(frames) >= 40
    assert {a.shape[2] for a in frames} == {1, 3, 4}
    ims = [gpu.Image(a) for a in frames]
    vals, codes, launches = gpu.batch_calc_perceived_brightness(ims)
    lone = lone_values(gpu, ims)
    print("launches", launches)
    assert codes == [0] * len(frames)
    for a, got, alone in zip(frames, vals, lone):
        want = orc.brightness(a)
        assert f32(got) == f32(want), (a.shape, got, want)
        assert f32(got) == f32(alone), (a.shape, got, alone)
    assert launches <= 2 * 3, launches
    # the frames were only read
    for a, im in zip(frames[:12], ims[:12]):
        assert np.array_equal(im.numpy(), a)
    release(ims)


def test_launches_do_not_follow_the_count(gpu):
    rng = np.random.Generator(np.random.PCG64(0x1F0C))
    frames = [_noise(rng, 40 + 7 * i, 50 + 11 * i, 3) for i in range(64)]
    ims = [gpu.Image(a) for a in frames]
    vals, codes, launches = gpu.batch_calc_perceived_brightness(ims)
    assert codes == [0] * 64 and launches == 2, (codes, launches)
    for a, got in zip(frames, vals):
        assert f32(got) == f32(orc.brightness(a)), a.shape
    vals, codes, launches = gpu.batch_calc_perceived_brightness(ims[-1:])
    assert codes == [0] and launches == 2 and f32(vals[0]) == f32(orc.brightness(frames[-1]))
    release(ims)
    small = [_noise(rng, 16 + i, 257 - 16 * i, 3) for i in range(8)]        # 4112 pixels at most
    assert max(a.shape[0] * a.shape[1] for a in small) == 4112
    ims = [gpu.Image(a) for a in small]
    vals, codes, launches = gpu.batch_calc_perceived_brightness(ims)
    assert codes == [0] * 8 and launches == 1, (codes, launches)
    for a, got in zip(small, vals):
        assert f32(got) == f32(orc.brightness(a)), a.shape
    vals, codes, launches = gpu.batch_calc_perceived_brightness([])
    assert (vals, codes, launches) == ([], [], 0)
    release(ims)


def test_per_entry_verdicts_brightness(gpu):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1F0D))
    frames = [_noise(rng, 90, 130, 3), _gray_equal(rng, 200, 300, 4), _flat100(rng, 70, 80, 1), _noise(rng, 33, 47, 4), _zero_prefix(rng, 150, 150, 3)]
    want = [orc.brightness(a) for a in frames]
    ims = [gpu.Image(a) for a in frames]
    # a NULL handle in the middle
    with_null = ims[:2] + [None] + ims[2:]
    vals, codes, _ = gpu.batch_calc_perceived_brightness(with_null)
    assert codes == [0, 0, INVALID, 0, 0, 0]
    assert [f32(v) for v in vals[:2] + vals[3:]] == [f32(v) for v in want]
    # brightness only reads: the same handle may come twice
    vals, codes, _ = gpu.batch_calc_perceived_brightness([ims[0], ims[1], ims[0]])
    assert codes == [0, 0, 0] and f32(vals[0]) == f32(vals[2]) == f32(want[0])
    # the fault point of the lone call, entered per valid entry in entry order: the third VALID entry fails, alone
    lib = gpu.lib
    try:
        assert lib.impgpu_fault_arm(STEP_INFO, 3) == 0
        vals, codes, _ = gpu.batch_calc_perceived_brightness(with_null)
        assert lib.impgpu_fault_arm(STEP_INFO, 3) == 0
        loop = []
        for im in with_null:
            if im is None:
                loop.append(INVALID)
                continue
            try:
                im.calc_perceived_brightness()
                loop.append(0)
            except gpu.ImpError as e:
                loop.append(e.code)
    finally:
        lib.impgpu_fault_arm(-1, 0)
    assert codes == [0, 0, INVALID, DEVICE, 0, 0] and codes == loop, (codes, loop)
    assert vals[3] is None
    assert [f32(v) for v in vals[:2] + vals[4:]] == [f32(v) for v in want[:2] + want[3:]]
    # an album gives frame 0; a cropped view (step > w * c) and wrapped memory are frames like any other
    album = gpu.Image.album([frames[0], _noise(rng, 90, 130, 3)])
    big = _noise(rng, 120, 200, 3)
    base = gpu.Image(big)
    x, y, w, h = 13, 9, 150, 100
    view = gpu.Image.wrap(base.device_ptr + y * base.step + x * 3, w, h, 3, base.step)
    assert view.step > w * 3
    raw = _dark_then_bright(rng, 77, 101, 4)
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    wrapped = gpu.Image.wrap(t.data_ptr(), 101, 77, 4, 101 * 4)
    vals, codes, launches = gpu.batch_calc_perceived_brightness([album, view, wrapped])
    assert codes == [0, 0, 0] and launches <= 4
    assert f32(vals[0]) == f32(want[0]) == f32(album.calc_perceived_brightness())
    assert f32(vals[1]) == f32(orc.brightness(np.ascontiguousarray(big[y:y + h, x:x + w]))) == f32(view.calc_perceived_brightness())
    assert f32(vals[2]) == f32(orc.brightness(raw)) == f32(wrapped.calc_perceived_brightness())
    release([album, view, wrapped, base], ims)
    del t


ASCII_SIZES = [(1, 1), (2, 3), (60, 45), (224, 224), (640, 480)]            # (width, height)
ASCII_ARGS = ["", "wide", None, "narrowish"]                                 # an unknown word is the narrow table, as impgpu_ascii


def ascii_pool():
    rng = np.random.Generator(np.random.PCG64(0x1F0E))
    frames, args = [], []
    k = 0
    for (w, h) in ASCII_SIZES:
        for c in (3, 4):
            for rep in range(2):
                frames.append(_noise(rng, h, w, c) if (k + rep) % 2 else smooth_image(h, w, c, k)[:, :, :c])
                args.append(ASCII_ARGS[k % len(ASCII_ARGS)])
                k += 1
    return frames, args


def test_ascii_batch(gpu):
    frames, args = ascii_pool()
    assert len(frames) >= 16
    ims = [gpu.Image(a) for a in frames]
    clones = [im.clone() for im in ims]
    texts, codes, launches = gpu.batch_ascii(ims, args)
    assert codes == [0] * len(frames) and launches <= 2, (codes, launches)
    for a, arg, im, cl, got in zip(frames, args, ims, clones, texts):
        assert got == orc.ascii_art(a, arg or ""), (a.shape, arg)
        assert got == cl.ascii(arg or ""), (a.shape, arg)
        after = im.numpy()
        assert np.array_equal(after, cl.numpy()), a.shape                    # HSV in place, alpha untouched
        assert np.array_equal(after[:, :, :3], orc.rgb2hsv(np.ascontiguousarray(a[:, :, :3])))
        if a.shape[2] == 4:
            assert np.array_equal(after[:, :, 3], a[:, :, 3])
    release(ims, clones)
    # args itself may be NULL: every text narrow
    ims = [gpu.Image(a) for a in frames[:5]]
    texts, codes, launches = gpu.batch_ascii(ims, None)
    assert codes == [0] * 5
    assert texts == [orc.ascii_art(a, "") for a in frames[:5]]
    release(ims)


def test_ascii_per_entry_verdicts(gpu):
    import ctypes as C

    rng = np.random.Generator(np.random.PCG64(0x1F0F))
    frames = [_noise(rng, 30, 40, 3), _noise(rng, 25, 35, 1), _noise(rng, 20, 50, 4), _noise(rng, 45, 60, 3), _noise(rng, 10, 10, 4)]
    ims = [gpu.Image(a) for a in frames]
    n = len(ims)
    need = [(a.shape[1] + 1) * a.shape[0] - 1 for a in frames]
    caps = list(need)
    caps[3] = need[3] - 1                                                    # one byte short
    bufs = [(C.c_ubyte * (k + 8))(*([0xA5] * (k + 8))) for k in need]
    handles = (C.c_void_p * n)(*[im.h.value for im in ims])
    handles[4] = None                                                        # and a NULL handle
    cargs = (C.c_char_p * n)(b"", b"wide", None, b"wide", b"")
    outs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    ccaps = (C.c_long * n)(*caps)
    lens = (C.c_long * n)(*([-7] * n))
    codes = (C.c_int * n)(*([-1] * n))
    launches = C.c_int(-1)
    assert gpu.lib.impgpu_batch_ascii(handles, cargs, n, outs, ccaps, lens, codes, C.byref(launches)) == 0
    assert list(codes) == [0, INVALID, 0, INVALID, INVALID] and launches.value == 2
    for i in (0, 2):
        assert lens[i] == need[i]
        assert bytes(bufs[i][:need[i]]) == orc.ascii_art(frames[i], "")
        assert bytes(bufs[i][need[i]:]) == b"\xa5" * 8                       # nothing past the text
    for i in (1, 3, 4):                                                      # refused: buffer, length and frame untouched
        assert bytes(bufs[i]) == b"\xa5" * (need[i] + 8) and lens[i] == -7
    assert np.array_equal(ims[1].numpy(), frames[1]) and np.array_equal(ims[3].numpy(), frames[3]) and np.array_equal(ims[4].numpy(), frames[4])
    # a NULL outs[i]
    fresh = [gpu.Image(frames[0]), gpu.Image(frames[2])]
    h2 = (C.c_void_p * 2)(fresh[0].h.value, fresh[1].h.value)
    o2 = (C.c_void_p * 2)(None, C.addressof(bufs[2]))
    c2 = (C.c_long * 2)(need[0], need[2])
    l2 = (C.c_long * 2)()
    k2 = (C.c_int * 2)()
    assert gpu.lib.impgpu_batch_ascii(h2, None, 2, o2, c2, l2, k2, None) == 0
    assert list(k2) == [INVALID, 0] and np.array_equal(fresh[0].numpy(), frames[0])
    # the same handle twice: refused as a whole, no frame changed
    again = [gpu.Image(frames[0]), gpu.Image(frames[3])]
    with pytest.raises(gpu.ImpError) as e:
        gpu.batch_ascii([again[0], again[1], again[0]], ["", "", "wide"])
    assert e.value.code == INVALID
    assert np.array_equal(again[0].numpy(), frames[0]) and np.array_equal(again[1].numpy(), frames[3])
    release(ims, fresh, again)


def test_threads_each_on_its_own_lane(gpu):
    """Four threads, each a lane of its own (stream, pool, pinned staging), each making batch calls over frames it made."""
    rng = np.random.Generator(np.random.PCG64(0x1F10))
    jobs = []
    for t in range(4):
        frames = [CONTENTS[(t + i) % len(CONTENTS)](rng, 30 + 41 * i + 3 * t, 50 + 37 * i + 5 * t, (3, 4, 1, 3, 4, 3)[(i + t) % 6]) for i in range(10)]
        colour = [a for a in frames if a.shape[2] >= 3]
        jobs.append((frames, [orc.brightness(a) for a in frames], colour, [orc.ascii_art(a, "wide" if i % 2 else "") for i, a in enumerate(colour)]))
    errors = []
    gate = threading.Barrier(4)

    def work(t):
        try:
            frames, want, colour, want_text = jobs[t]
            gate.wait(timeout=60)
            for rep in range(6):
                ims = [gpu.Image(a) for a in frames]
                vals, codes, launches = gpu.batch_calc_perceived_brightness(ims)
                assert codes == [0] * len(frames) and launches <= 6, (t, rep, codes, launches)
                assert [f32(v) for v in vals] == [f32(v) for v in want], (t, rep)
                cims = [gpu.Image(a) for a in colour]
                texts, codes, launches = gpu.batch_ascii(cims, ["wide" if i % 2 else "" for i in range(len(colour))])
                assert codes == [0] * len(colour) and launches <= 2, (t, rep, codes, launches)
                assert texts == want_text, (t, rep)
                for a, im in zip(colour, cims):
                    assert np.array_equal(im.numpy()[:, :, :3], orc.rgb2hsv(np.ascontiguousarray(a[:, :, :3]))), (t, rep, a.shape)
                release(ims, cims)
        except BaseException as e:                                           # noqa: BLE001 -- reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not errors, errors
    assert not any(th.is_alive() for th in threads)
