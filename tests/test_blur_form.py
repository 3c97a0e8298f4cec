"""impgpu_blur_form: which Gaussian form a frame gets for a sigma (host only, no device) -- the sweep the batched tests take
their sigmas from."""
import ngx_http_imgproc_amd as imp
from test_gpu_blur_wide_mix import SIGMA_PAIR_2, SIGMAS_ONE_PASS, SIGMAS_PAIR_2_MORE, SIGMAS_PAIR_3

SIGMAS = [k / 10 for k in range(5, 251)]           # 0.5 .. 25.0 in steps of 0.1


def _sweep(c):
    return [(s,) + imp.blur_form(200, 150, c, s) for s in SIGMAS]


def test_forms_are_monotone_in_sigma():
    """1 / 2 (one pass), then 3 (two passes), then 0, and never back.  Across ALL sigmas that holds for each byte-plane count
    by itself, not for the two mingled: the one-pass matrix-unit form ends where its tile passes 40 KB of LDS with two byte
    planes but 50 KB with three, so BGR at sigma 7.3 (three planes, one pass) follows sigma 6.6 .. 7.2 (two planes, two
    passes).  Form 1 and form 0 have no planes and bound both sequences."""
    rank = {1: 0, 2: 0, 3: 1, 0: 2}
    for c in (3, 4):
        sweep = _sweep(c)
        assert all(f in rank for _, f, _ in sweep)
        assert all((p in (2, 3)) == (f in (2, 3)) and (p == 0) == (f in (0, 1)) for _, f, p in sweep), c
        for planes in (2, 3):
            ranks = [rank[f] for _, f, p in sweep if p in (0, planes)]
            assert ranks == sorted(ranks), (c, planes)
        assert sweep[0][1] == 1                                          # sigma 0.5: kernel size 5, k_blur_fused4
        two_pass = [s for s, f, _ in sweep if f == 3]
        assert two_pass and all(f in (3, 0) for s, f, _ in sweep if s > 10.5), c
        print(c, "two passes from sigma", two_pass[0], "three planes at", [s for s, f, p in sweep if f == 3 and p == 3])


def test_headline_sigma_is_two_pass_and_sigma_4_is_wide():
    for c in (3, 4):
        assert imp.blur_form(200, 150, c, 8.0) == (3, 2)
        assert imp.blur_form(200, 150, c, 4.0)[1] == 3
        assert imp.blur_form(1920, 1080, c, 8.0) == (3, 2)              # the form does not follow the frame's size ...
    assert imp.blur_form(200, 1, 3, 8.0) == (0, 0)                      # ... but 1-pixel axes and other channel counts are lone
    assert imp.blur_form(200, 150, 1, 8.0) == (0, 0)
    assert imp.blur_form(200, 150, 4, 0.0) == (0, 0)                    # no blur at all
    assert imp.lib.impgpu_blur_form(200, 150, 4, 8.0, None) == 3        # planes may be NULL


def test_the_gpu_tests_sigmas_are_what_they_say():
    for c in (3, 4):
        for s in (SIGMA_PAIR_2,) + SIGMAS_PAIR_2_MORE:
            assert imp.blur_form(200, 150, c, s) == (3, 2), (c, s)
        for s in SIGMAS_ONE_PASS:
            assert imp.blur_form(200, 150, c, s) == (2, 2), (c, s)
        for s in SIGMAS_PAIR_3:
            assert imp.blur_form(200, 150, c, s) == (3, 3), (c, s)
