"""Every descriptor class of launch_resize_mixed in one call per channel count: a characterisation of the dispatcher.

A call holds two frames of each class its channel count has -- general AREA rows, four columns per lane, BGR rows that are
not 4-byte aligned (cells), whole factors, wide cells -- and one CUBIC enlargement, which goes alone, interleaved; a second
call with `simple` set holds three NN frames.  Every output must equal, byte for byte, what one impgpu_batch_cv_resize
launch per frame leaves and what the oracle computes, and the number of kernels enqueued is the one the library reported
before the dispatcher was taken apart (measured then, written down here): a frame that changed class would change it."""
import numpy as np
import pytest

import oracle_lib as orc
from test_gpu_gray_mix import widest_cell
from test_gpu_int_mix import CANARY, Frame, _check_frames

pytestmark = pytest.mark.gpu

A, CUBIC, NN = orc.INTER_AREA, orc.INTER_CUBIC, orc.INTER_NN
# class -> two shapes (sw, sh, dw, dh)
ROWS = [(97, 61, 40, 25), (120, 50, 33, 21)]              # windows of 4: dw < 160 keeps one column per lane
ROWS4 = [(401, 90, 170, 38), (500, 70, 200, 30)]          # windows of at most 5 and dw >= 160: four columns per lane
CELLS = [(97, 61, 40, 25), (150, 40, 31, 9)]              # as ROWS, from BGR rows off the 4-byte grid
WHOLE = [(64, 48, 32, 24), (96, 60, 32, 20)]              # 2 x 2 and 3 x 3
WIDE = [(700, 64, 24, 7), (900, 41, 30, 5)]               # cells of 30 columns; (900 x 40 -> 30 x 5 would be a whole 30 x 8)
LONE = (20, 20, 33, 31)
# kernels enqueued, as the library reported them before the refactor of the dispatcher (and reports them since): the rows of
# every kind share k_resize_area_mix, the whole factors k_area_int_mix, the wide cells k_resize_area_wide_mix, and the
# enlargement has its own launch; gray frames have no wide class
LAUNCHES = {1: 3, 3: 4, 4: 4}
LAUNCHES_SIMPLE = 1                                       # three NN frames: k_resize_nn_mix


def test_the_shapes_are_what_they_claim():
    def whole(sw, sh, dw, dh):
        return sw % dw == 0 and sh % dh == 0

    assert all(whole(*s) for s in WHOLE) and not any(whole(*s) for s in ROWS + ROWS4 + CELLS + WIDE)
    assert all(widest_cell(sw, dw) <= 20 and dw < 160 for sw, _, dw, _ in ROWS + CELLS)
    assert all(2 <= widest_cell(sw, dw) <= 5 and dw >= 160 for sw, _, dw, _ in ROWS4)
    assert all(21 <= widest_cell(sw, dw) <= 66 for sw, _, dw, _ in WIDE)
    assert LONE[2] > LONE[0]                              # an enlargement: CUBIC (bridge.c:188-192)


class Placed(Frame):
    """test_gpu_int_mix.Frame with the alignment of its source rows chosen, not drawn: on the 4-byte grid, or off it."""

    def __init__(self, torch, rng, cn, shape, interp, aligned=True):
        sw, sh, dw, dh = shape
        self.cn, self.sw, self.sh, self.dw, self.dh, self.interp = cn, sw, sh, dw, dh, interp
        ox, oy, py, dpad = (4 if aligned else 1), int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(0, 4))
        px = (-(sw + ox)) % 4 + (0 if aligned else 1)
        self.host = rng.integers(0, 256, size=(sh + oy + py, sw + ox + px, cn), dtype=np.uint8)
        self.window = self.host[oy:oy + sh, ox:ox + sw]
        self.src = torch.from_numpy(self.host).cuda()
        self.sstep = self.host.shape[1] * cn
        self.sptr = self.src.data_ptr() + oy * self.sstep + ox * cn
        assert cn != 3 or aligned == (self.sptr % 4 == 0 and self.sstep % 4 == 0)
        self.dsts = [torch.full((dh, dw + dpad, cn), CANARY, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.dstep = (dw + dpad) * cn


def _interleaved(classes):
    """The first frame of every class, then the second ones."""
    return [c[k] for k in range(2) for c in classes]


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_every_class_in_one_call(gpu, cn):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DA100 + cn))
    classes = [[Placed(torch, rng, cn, s, A) for s in shapes] for shapes in ([ROWS, ROWS4, WHOLE] + ([WIDE] if cn != 1 else []))]
    if cn == 3:
        classes.append([Placed(torch, rng, cn, s, A, aligned=False) for s in CELLS])
    frames = _interleaved(classes)
    frames.insert(len(frames) // 2, Placed(torch, rng, cn, LONE, CUBIC))
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, count_launches=True)
    print("cn %d: %d frames, %d launches" % (cn, len(frames), launches))
    assert rc == 0
    _check_frames(gpu, frames, cn, "every class")
    assert launches == LAUNCHES[cn], launches


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_three_nn_frames(gpu, cn):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DA200 + cn))
    frames = [Placed(torch, rng, cn, s, NN) for s in (ROWS[0], WHOLE[0], LONE)]
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, simple=True, count_launches=True)
    print("cn %d simple: %d frames, %d launches" % (cn, len(frames), launches))
    assert rc == 0
    _check_frames(gpu, frames, cn, "simple")
    assert launches == LAUNCHES_SIMPLE, launches
