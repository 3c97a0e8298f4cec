"""The boundary fixtures of webp_dec_cases.boundary_cases() (tests/golden/webp_dec/h_b_*.webp) reach the seams of the
decoder they were written for (no device).  What a file holds comes from the WRITER -- its token list, the code lengths
it put out, its model of the round rule (webp_dec_cases.RoundModel) -- and is held against the host model's info words:
[6] the rounds the main image took, [7] the longest code length among its codes, [0] the feature word, [1] the groups,
[2] the cache bits, [4] the coded width.  That every file decodes to Pillow's frame is test_webp_decode_host.py's, which
takes the whole directory.

WHAT THE 223 FIXTURES BEFORE THESE REACHED (test_what_the_earlier_fixtures_reached prints and pins it):
  * more than 256 rows WITH a predictor (a second band of k_webp_dec_inverse): none.  p_flat_300x300_m0/3/6 have 300 rows and
    no predictor: colour indexing at eight pixels a value is their only transform.
  * a code longer than the 10-bit table: nine Pillow files -- p_photo_53x37_m0/3, p_rgba_53x37_m0/3/6 and
    p_tiling_318x222_m0/3 with 11 bits, p_photo_53x37_m6 and p_tiling_318x222_m6 with 12.  No hand-written file, nothing
    past 12 bits.
  * a round that ended on the staged window and not on the token count: none.  (info[] does not say how a round ended; this
    was measured once with the host loop of wd_rounds_host counting the rounds that ended with fewer than 512 tokens in
    front of the image's end.  Of all 301 files only h_b_a3_64x48, 10 of 11 rounds, and h_b_a3_260x130, 13 of 14, do.)
"""
import webp_dec_cases as cases
import webp_dec_fixtures as F
from ngx_http_imgproc_amd import ops

PREDICTOR, COLOR, SUB_GREEN, INDEXING, CACHE, GROUPS, BACKREF = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
FAMILIES = {"A1": 5, "A2": 6, "A3": 2, "B": 22, "C": 20, "D": 12, "E": 2, "F": 5, "G": 4}
FAST = 10                                         # WD_FAST: bits of a code's lookup table
_INFO = {}


def info_of(name):
    """the host model's info words for h_<name>.webp, decoded once"""
    if name not in _INFO:
        rc, _, info, intact = ops.webp_decode_host(F.read("h_" + name + ".webp"))
        assert rc == F.IMP_OK and intact, name
        _INFO[name] = info
    return _INFO[name]


def family(which):
    out = {name: facts for name, facts in cases.boundary_facts().items() if facts["family"] == which}
    assert len(out) == FAMILIES[which], (which, sorted(out))
    return out


def rounds_by_count(facts):
    return -(-facts["tokens"] // cases.TOKENS)


def test_the_committed_files_are_what_the_writer_writes_and_every_family_is_there():
    written = cases.boundary_cases()
    assert len(written) == sum(FAMILIES.values()) == len(cases.boundary_facts())
    for name, blob in written:
        assert name.startswith("b_") and len(blob) < 65536 and F.read("h_" + name + ".webp") == blob, name
    assert {name for name, _, _ in F.load() if name.startswith("h_b_")} == {"h_" + name for name, _ in written}
    # cases() keeps its files and its order
    assert [name for name, _ in cases.cases()][:3] == ["mode00", "mode01", "mode02"] and len(cases.cases()) == 154
    for name, blob in cases.cases():
        assert F.read("h_" + name + ".webp") == blob, name


def test_rounds_and_longest_code_are_the_writers_for_every_file():
    """info[6] against the round model fed with the bits the writer put out, info[7] against the lengths it wrote"""
    wrong = [(name, info_of(name)[6:8], facts["rounds"], facts["maxlen"]) for name, facts in cases.boundary_facts().items()
             if info_of(name)[6] != facts["rounds"] or info_of(name)[7] != facts["maxlen"]]
    assert not wrong, wrong


def test_a1_the_token_count_ends_the_round():
    fam = family("A1")
    rounds = {}
    for name, facts in fam.items():
        assert facts["height"] == 1 and facts["tokens"] == facts["width"] and facts["window_rounds"] == 0 and facts["maxlen"] <= 4, name
        assert info_of(name)[6] == rounds_by_count(facts), name
        rounds[facts["width"]] = info_of(name)[6]
    assert rounds == {511: 1, 512: 1, 513: 2, 1024: 2, 1025: 3}


def test_a2_a_match_is_token_512_and_token_513():
    fam = family("A2")
    at = {}
    for name, facts in fam.items():
        assert (facts["width"], facts["height"]) == (520, 2) and facts["window_rounds"] == 0
        info = info_of(name)
        assert info[6] == rounds_by_count(facts) and info[0] & BACKREF and info[2] == (4 if name.endswith("c4") else 0), name
        at[name] = facts["match_token"]
    # without a cache the tokens in front are literals, one a pixel: the match is the round's last token, the next round's
    # first, and in the middle of a round (with a cache the cache tokens in front are one a pixel too)
    assert at == {"b_a2_tok512_c0": 511, "b_a2_tok513_c0": 512, "b_a2_mid_c0": 300, "b_a2_tok512_c4": 511, "b_a2_tok513_c4": 512, "b_a2_mid_c4": 300}


def test_a3_the_window_ends_the_round_with_15_bit_codes():
    fam = family("A3")
    for name, facts in fam.items():
        info = info_of(name)
        assert info[6] > rounds_by_count(facts) and info[7] == 15, (name, info)
        assert facts["window_rounds"] >= info[6] - rounds_by_count(facts) and facts["window_rounds"] == len(facts["last_of_window"])
    # the placed tokens: a match of the longest token there is as the LAST token of a window-ended round, a match that
    # reaches back to pixel 0 as the FIRST of the next; seven of 4096 pixels, and one distance past 32768
    facts = fam["b_a3_260x130"]
    longs = [(tok, pos) for kind, tok, pos in facts["placed"] if kind == "long"]
    fars = [(tok, pos) for kind, tok, pos in facts["placed"] if kind == "far"]
    assert len(longs) == len(fars) >= 8 and all(tok in facts["last_of_window"] for tok, _ in longs)
    assert [tok for tok, _ in fars] == [tok + 1 for tok, _ in longs]
    assert sum(1 for (_, a), (_, b) in zip(longs, fars) if b - a == 4096) >= 7 and max(pos for _, pos in fars) > 32768
    assert info_of("b_a3_260x130")[0] & BACKREF and not info_of("b_a3_64x48")[0] & BACKREF


def test_b_every_length_at_the_waves_width_with_and_without_a_cache():
    fam = family("B")
    assert sorted({f["length"] for f in fam.values()}) == [1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096]
    assert sorted({(f["length"], f["cache_bits"]) for f in fam.values() if f["cache_bits"]}) == [(n, b) for n in (2, 64, 65, 4096) for b in (1, 6, 11)]
    for name, facts in fam.items():
        info = info_of(name)
        assert info[0] & BACKREF and info[2] == facts["cache_bits"] and bool(info[0] & CACHE) == bool(facts["cache_bits"]), name


def test_c_a_second_band_of_rows_with_a_predictor():
    fam = family("C")
    shapes = {(f["width"], f["height"]) for name, f in fam.items() if name[4].isdigit()}
    assert shapes == {(w, h) for w in (1, 2, 3, 5) for h in (255, 256, 257, 513)}
    for name, facts in fam.items():
        assert info_of(name)[0] & PREDICTOR, name
    assert sum(1 for f in fam.values() if f["height"] > 256) == 12 and sum(1 for f in fam.values() if f["height"] > 512) == 5
    assert info_of("b_c_pcg_3x257")[0] & (PREDICTOR | COLOR | SUB_GREEN) == PREDICTOR | COLOR | SUB_GREEN and info_of("b_c_pcg_3x257")[3] == 3


def test_d_the_longest_code_is_the_one_written():
    fam = family("D")
    for what in ("green", "red", "blue", "alpha", "dist"):
        assert info_of("b_d_%s_10_11" % what)[7] == 11 == fam["b_d_%s_10_11" % what]["maxlen"], what
        assert info_of("b_d_%s_15" % what)[7] == 15 == fam["b_d_%s_15" % what]["maxlen"], what
    assert info_of("b_d_dist_15")[0] & BACKREF and info_of("b_d_dist_10_11")[0] & BACKREF
    assert info_of("b_d_cache_top")[2] == 11 and fam["b_d_cache_top"]["top_key"] == 2
    assert fam["b_d_dist39"]["far"] + 120 > 786432 and info_of("b_d_dist39")[0] & BACKREF       # distance symbol 39: codes 786433..1048576


def test_e_324_groups():
    for name, facts in family("E").items():
        info = info_of(name)
        assert info[1] == 324 == facts["groups"] and info[0] & GROUPS and info[0] & BACKREF and facts["crossing"] > 100, name
    assert info_of("b_e_groups324_c3")[2] == 3 and info_of("b_e_groups324_c0")[2] == 0


def test_f_the_largest_sides():
    fam = family("F")
    for name in ("b_f_pcg_16383x1", "b_f_pcg_1x16383"):
        assert info_of(name)[0] & 7 == 7 and info_of(name)[3] == 3 and max(fam[name]["width"], fam[name]["height"]) == 16383, name
    assert info_of("b_f_pal2_16383x1")[4] == 2048 and info_of("b_f_pal2_16383x1")[0] & 0x2000
    assert info_of("b_f_pal4_1x300")[4] == 1 and info_of("b_f_pal4_1x300")[0] & 0x1000
    assert info_of("b_f_pal16_1x300")[4] == 1 and info_of("b_f_pal16_1x300")[0] & 0x0800


def test_g_sub_images_with_matches_and_a_cache_of_their_own():
    """the main image of these files has no cache (info[2]) and only literals: the cache and backward-reference bits come
    from a sub-image"""
    for name, facts in family("G").items():
        info = info_of(name)
        assert info[2] == 0 and info[0] & CACHE and info[0] & BACKREF, (name, info)
        assert info[1] == facts.get("groups", 1), name
    assert info_of("b_g_predictor")[0] & PREDICTOR and info_of("b_g_colour")[0] & COLOR and info_of("b_g_meta")[0] & GROUPS
    assert info_of("b_g_all")[0] & (PREDICTOR | COLOR | SUB_GREEN | GROUPS) == PREDICTOR | COLOR | SUB_GREEN | GROUPS


def test_what_the_earlier_fixtures_reached(capsys):
    """the module docstring's record, measured: printed, and pinned so that it cannot go stale"""
    tall, long_codes = [], {}
    for name, blob, expected in F.load():
        if name.startswith("h_b_"):
            continue
        rc, _, info, _ = ops.webp_decode_host(blob)
        assert rc == F.IMP_OK, name
        if expected.shape[0] > 256 and info[0] & PREDICTOR:
            tall.append(name)
        if info[7] > FAST:
            long_codes[name] = info[7]
    with capsys.disabled():
        print("\nearlier fixtures with more than 256 rows and a predictor:", tall or "none")
        print("earlier fixtures with a code longer than 10 bits:", long_codes or "none")
    assert tall == []
    assert long_codes == {"p_photo_53x37_m0": 11, "p_photo_53x37_m3": 11, "p_photo_53x37_m6": 12, "p_rgba_53x37_m0": 11, "p_rgba_53x37_m3": 11,
                          "p_rgba_53x37_m6": 11, "p_tiling_318x222_m0": 11, "p_tiling_318x222_m3": 11, "p_tiling_318x222_m6": 12}
