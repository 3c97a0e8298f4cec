"""IMPGPU_GIF_SPLIT against the one-wave route and the host decoder, in one session on the same files: for every canvas, page
count and file count of tools/gif_decode_probe.py (its files: Pillow's encoder writes each page's LZW stream), and for a
photo-like 640 x 480 page and a 1920 x 1080 page (smooth gradients plus noise, tests/gif_writer.py's encoder),

    flags = 0                  impgpu_batch_decode_gif_ex: k_gif_lzw, one wavefront per page, + k_gif_compose_mix
    flags = IMPGPU_GIF_SPLIT   k_gif_lzw_scan / _len / _emit, one wavefront per segment, + k_gif_compose_mix
    host                       impgpu_gif_pages(how = 0) for every file on ONE thread: the LZW alone, no compose, no upload

Times are wall time from the call to the end of the device's work (impgpu_sync inside the timed region), medians over
--iters calls after a warm-up call, microseconds; every route is timed in two halves with the others in between, and both
halves are written down.  "segments" is what impgpu_gif_pages_split counts for the file's pages.  A row whose planes and
albums would pass --max-gb of device memory is written with "skipped".

    timeout -k 10 900 python tools/gif_split_probe.py [--iters 7] [--out profiles/gif_split_probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch  # noqa: F401  (first: the HIP runtime torch bundles, as in bench.py)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gif_decode_probe import FILES, PAGES, SIZES, make_file, median_us  # noqa: E402


def photo_file(w, h, seed):
    """one page of smooth gradients plus noise, 256 colours: what a dithered photograph looks like to LZW"""
    import gif_writer as G

    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    idx = ((xx + 2 * yy) // 6 + rng.integers(0, 12, (h, w))).astype(np.uint8)
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    return G.write([G.make_page(idx, palette=pal, mcs=8)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--max-gb", type=float, default=3.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gif_split_probe.json"))
    a = ap.parse_args()
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    cases = [("probe", w, h, pages, files) for w, h in SIZES for pages in PAGES for files in FILES]
    cases += [("photo", 640, 480, 1, 1), ("photo", 640, 480, 1, 8), ("photo", 1920, 1080, 1, 1)]
    made = {}
    rows = []
    for kind, w, h, pages, files in cases:
        key = (kind, w, h, pages)
        if key not in made:
            made[key] = make_file(w, h, pages, 100 + pages) if kind == "probe" else photo_file(w, h, 7)
        blob = made[key]
        plane = ((w + 3) & ~3) * h * pages
        rc, _, segs = imp.gif_pages_split(blob)
        assert rc == 0, rc
        row = {"probe": "gif_split", "content": kind, "canvas": [w, h], "pages": pages, "files": files, "file_bytes": len(blob), "plane_bytes": plane,
               "segments_per_file": sum(segs), "segments_most": max(segs), "min_bytes": imp.GIF_SPLIT_MIN_BYTES, "iters": a.iters}
        if files * plane * 5 > a.max_gb * (1 << 30):
            row["skipped"] = "planes and albums of %d files pass %.1f GB" % (files, a.max_gb)
            rows.append(row)
            print(json.dumps(row), flush=True)
            continue
        blobs = (C.c_char_p * files)(*[blob] * files)
        sizes = (C.c_size_t * files)(*[len(blob)] * files)
        destr, which = (C.c_int * files)(*[1] * files), (C.c_int * files)(*[-1] * files)
        outs, codes, launches = (C.c_void_p * files)(), (C.c_int * files)(), C.c_int()
        out = np.zeros(plane, np.uint8)
        n = C.c_size_t()

        def device(flags, want):
            def run():
                rc = imp.lib.impgpu_batch_decode_gif_ex(blobs, sizes, destr, which, files, flags, outs, codes, C.byref(launches))
                assert rc == 0 and not any(codes) and launches.value == want, (rc, list(codes), launches.value)
                imp.sync()
                for i in range(files):
                    imp.lib.impgpu_image_release(C.byref(C.c_void_p(outs[i])))
            return run

        def host():
            for _ in range(files):
                rc = imp.lib.impgpu_gif_pages(blob, len(blob), 0, out.ctypes.data, plane, C.byref(n))
                assert rc == 0, rc

        one, split = device(0, 2), device(imp.GIF_SPLIT, 4)
        h1, h2 = a.iters // 2, a.iters - a.iters // 2
        o1, s1, c1 = median_us(one, h1), median_us(split, h1), median_us(host, h1)
        c2, s2, o2 = median_us(host, h2), median_us(split, h2), median_us(one, h2)
        row.update({"one_wave_us": round((o1 + o2) / 2, 1), "split_us": round((s1 + s2) / 2, 1), "host_lzw_us": round((c1 + c2) / 2, 1),
                    "one_wave_halves_us": [round(o1, 1), round(o2, 1)], "split_halves_us": [round(s1, 1), round(s2, 1)],
                    "host_halves_us": [round(c1, 1), round(c2, 1)], "split_over_one_wave": round((o1 + o2) / (s1 + s2), 3),
                    "split_over_host": round((c1 + c2) / (s1 + s2), 3),
                    "host_decoder": "impgpu_gif_pages(how=0), one thread, LZW only (FreeImage is not installed)"})
        rows.append(row)
        print(json.dumps(row), flush=True)
    imp.env_destroy()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
