"""impgpu_batch_decode_png_ex on 64 files of 640x480 palette (depth 8) and 64 of 1920x1080 Adam7 RGB: the wall time of one
batch call against 64 single calls, and Pillow's host decode of the same files on one core.  One JSON line per set.
Run under `rocprofv3 --kernel-trace --stats -- python tools/png_ext_probe.py` for the kernels' times."""
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import png_ext_writer as W  # noqa: E402


def files(kind, n, seed):
    from ngx_http_imgproc_amd.workloads import photo_like

    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if kind == "palette":
            img = photo_like(480, 640, seed + k)[:, :, :3]
            pal = rng.integers(0, 256, size=(256, 3), dtype=np.uint8)
            idx = (img[:, :, 0] // 2 + img[:, :, 1] // 2).astype(np.uint8)
            out.append(W.write(idx[:, :, None], 3, 8, 0, kinds=lambda p, j: j % 5, palette=pal))
        else:
            img = photo_like(1080, 1920, seed + k)[:, :, :3]
            out.append(W.write(img, 2, 8, 1, kinds=lambda p, j: (p + j) % 5))
    return out


def main():
    import ngx_http_imgproc_amd as imp
    from PIL import Image

    imp.env_start(0)
    for kind in ("palette", "adam7_rgb"):
        blobs = files(kind, 64, 11)
        res, launches = imp.batch_decode_png_ex(blobs, imp.PNG_ALL)           # warm
        assert all(rc == 0 for rc, _ in res)
        for _, im in res:
            im.release()
        imp.sync()
        best_b = best_s = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            res, launches = imp.batch_decode_png_ex(blobs, imp.PNG_ALL)
            imp.sync()
            best_b = min(best_b, time.perf_counter() - t0)
            for _, im in res:
                im.release()
            t0 = time.perf_counter()
            ims = [imp.Image.decode_png_ex(b, imp.PNG_ALL)[1] for b in blobs]
            imp.sync()
            best_s = min(best_s, time.perf_counter() - t0)
            for im in ims:
                im.release()
        t0 = time.perf_counter()
        for b in blobs:
            Image.open(io.BytesIO(b)).load()
        pil = time.perf_counter() - t0
        print(json.dumps({"set": kind, "files": len(blobs), "bytes": sum(map(len, blobs)), "launches": launches,
                          "batch_ms": round(best_b * 1e3, 2), "singles_ms": round(best_s * 1e3, 2),
                          "pillow_one_core_ms": round(pil * 1e3, 2)}), flush=True)


if __name__ == "__main__":
    main()
