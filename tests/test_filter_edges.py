"""The in-loop filter kernels (csrc/deblock_kernels.hip, csrc/sao_kernels.hip) where tests/test_deblock.py, test_sao.py and test_filter_columns.py do not reach:

  geometry    every partial CTU extent from 8 to 56 samples in both directions, a 24-sample tail behind two whole CTU columns, pictures smaller than a CTU and a single
              unit row high (k_sao_stats stages a CTU in chunks of 16 samples with a per-sample tail and a per-sample path across the picture's edge; the other fixtures'
              partial CTUs are all 8 luma samples wide), through the picture-wide entry points and through the band and column forms, planes with poisoned margins, the
              statistics also with the planes' origins at an odd sample offset;
  deblocking  QP per CU over 0 .. 51 with the PPS offsets at the ends of their ranges (-6 .. 6, -12 .. 12): the table indices clip at both ends, the chroma QP mapping's
              min(qp - 6, 51) fires, tc reaches 24; content at the ends of the sample range (the filters' results clip at 0 and pmax) and with steps around the filters'
              thresholds; transquant bypass on and off, P and B records, each pass alone and both; an enumerated boundary-strength table
              (hevc_testlib.deblock_strength_rows) instead of random motion;
  SAO         offsets over the whole range (+-7, +-31 at 10 bits), content at the ends of the sample range (the offset sum clips both ways), band positions 28 .. 31 (the band
              index wraps), every type for luma and chroma, statistics of flat, checkerboard and saturated pictures.

Three levels as in the other filter tests: the oracle against the reference's own Deblock / SAO classes (oracle/_ref), the oracle against a committed digest
(tests/golden/filter_edges_golden.json, written by tests/golden/make_filter_edges_golden.py), the kernels against the oracle.  Integer paths: every comparison is exact.
The coverage conditions are asserted next to the digest, from the fixtures and the oracle's output alone, so that a fixture cannot stop reaching what it is there for.

What these tests were seen to catch (one change at a time to a scratch copy of the oracle, levels 1 and 2 at both depths; "old" = tests/test_sao.py, test_deblock.py,
test_filter_columns.py):
  caught here, missed by the old files: the beta index clipped at 50; the tc index without its 2 (bs - 1) at QP >= 50; the chroma QP mapping without its min(.., 51); the
      offset sum without its final clip; the normal and chroma filters' results clipped to -1 .. pmax or to 0 .. pmax + 1; coded residual counted on a prediction-only edge;
  caught here and by the old files: the band index without its & 31; the source samples of a CTU's columns beyond its last whole 16 taken as 0.
The same changes made to the kernels instead (beta index, chroma QP mapping, band index, tail columns; one run on an MI355X) fail level 3 here; the old GPU tests miss
the first two of them."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import hevc_testlib as T

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "filter_edges_golden.json")
needs_ref = pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built")

# ---------------------------------------------------------------- the cases ----------------------------------------------------------------
# deblocking, geometry: (seed, width, height, B records, bypass) -- deblock_case's ranges and content, the new widths and heights
DB_GEOMETRY = tuple((100 + i, w, h, bool(i & 1), i % 4 == 2) for i, (w, h) in enumerate(T.EDGE_GEOMETRIES))
# deblocking, parameters: on the 2x2-CTU geometries; (beta / 2, tc / 2, Cb, Cr) from the ends and the middle of the PPS ranges, opposite signs included
DB_OFFSETS = ((6, -6, 12, -12), (-6, 6, -12, 12), (6, 6, 12, 12), (-6, -6, -12, -12), (0, 0, 0, 0), (6, 0, 0, 12), (0, 6, 12, 0))
DB_STEPPED_QP = ((18, 27), (24, 34), (30, 40), (36, 46), (42, 52), (0, 52), (20, 52))


def _db_params():
    out = []
    for i, (w, h) in enumerate(T.EDGE_GEOMETRIES_2X2):
        out.append(dict(seed=200 + i, width=w, height=h, slice_b=bool(i & 1), bypass=i % 3 == 0, qp_range=(0, 52), content="saturated", offsets=DB_OFFSETS[i]))
        out.append(dict(seed=250 + i, width=w, height=h, slice_b=not (i & 1), bypass=i % 3 == 2, qp_range=(0, 52), content="saturated_rough", offsets=DB_OFFSETS[(i + 5) % 7]))
        out.append(dict(seed=300 + i, width=w, height=h, slice_b=not (i & 1), bypass=i % 3 == 1, qp_range=DB_STEPPED_QP[i], content="stepped", offsets=DB_OFFSETS[(i + 3) % 7]))
    return tuple(out)


DB_PARAMS = _db_params()
# SAO: (seed, width, height, keywords of sao_edge_case)
SAO_GEOMETRY = tuple((400 + i, w, h, dict(content="noise", index=i)) for i, (w, h) in enumerate(T.EDGE_GEOMETRIES))
SAO_PARAMS = tuple((500 + 2 * i + k, w, h, dict(content=("saturated", "noise")[k], index=2 * i + k, force_band=(28, 29, 30, 31) if (i + k) & 1 or not k else None))
                   for i, (w, h) in enumerate(T.EDGE_GEOMETRIES_2X2) for k in range(2))
SAO_STATS = tuple((600 + 3 * i + k, w, h, dict(content=("flat", "checker", "saturated")[k], source=("near", "near", "opposite")[k], index=3 * i + k))
                  for i, (w, h) in enumerate(T.EDGE_GEOMETRIES_2X2) for k in range(3))
SAO_GROUPS = dict(sao_geometry=SAO_GEOMETRY, sao_params=SAO_PARAMS, sao_stats=SAO_STATS)


def _name(c):
    return "%dx%d depth %d %s" % (c["width"], c["height"], c["depth"], c.get("content", ""))


@functools.lru_cache(maxsize=None)
def db_cases(depth, group):
    """[(case, passes to run)]"""
    if group == "deblock_geometry":
        return [(T.deblock_edge_case(depth, *g), (3,)) for g in DB_GEOMETRY]
    if group == "deblock_params":
        return [(T.deblock_edge_case(depth, **k), (1, 2, 3)) for k in DB_PARAMS]
    assert group == "deblock_strength"
    return [(T.deblock_strength_case(depth), (1, 2, 3))]


DB_GROUPS = ("deblock_geometry", "deblock_params", "deblock_strength")


@functools.lru_cache(maxsize=None)
def sao_cases(depth, group):
    return [T.sao_edge_case(depth, seed, w, h, **kw) for (seed, w, h, kw) in SAO_GROUPS[group]]


@functools.lru_cache(maxsize=None)
def db_oracle(depth, group):
    """the oracle's planes per (case, passes): computed once, read only"""
    O = T.load_oracle(depth)
    return [[T.deblock_run_host(O, c, p) for p in passes] for c, passes in db_cases(depth, group)]


@functools.lru_cache(maxsize=None)
def sao_oracle(depth, group):
    O = T.load_oracle(depth)
    return [T.sao_run_host(O, c) for c in sao_cases(depth, group)]


def digest(group, results):
    h = hashlib.sha256()
    for r in results:
        if group.startswith("deblock"):
            for planes in r:
                for p in planes:
                    h.update(p.tobytes())
        else:
            h.update(r[0].tobytes()); h.update(r[1].tobytes())
            for p in r[2]:
                h.update(p.tobytes())
    return h.hexdigest()


def _gold():
    with open(GOLD_PATH) as f:
        return json.load(f)


def _same_planes(got, want, what):
    for k in range(3):
        assert np.array_equal(got[k], want[k]), (what, T.edge_first_diff(got[k], want[k], k))


def _same_stats(got, want, what):
    for name, g, w in (("count", got[0], want[0]), ("offsetOrg", got[1], want[1])):
        if not np.array_equal(g, w):
            i = int(np.nonzero(g != w)[0][0])
            raise AssertionError((what, name, "ctu %d plane %d type %d class %d" % (i // 480, i // 160 % 3, i // 32 % 5, i % 32), int(g[i]), int(w[i])))


# ---------------------------------------------------------------- level 1: the oracle against the reference ----------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("group", DB_GROUPS)
@pytest.mark.parametrize("depth", [8, 10])
def test_deblock_oracle_vs_reference(depth, group):
    R = T.load_ref(depth)
    for (c, passes), wants in zip(db_cases(depth, group), db_oracle(depth, group)):
        for p, want in zip(passes, wants):
            got = T.deblock_run_host(R, c, p)
            _same_planes(got, want, (_name(c), "passes %d" % p))
            T.edge_margins_intact(depth, got, c["width"], c["height"], (_name(c), "reference"))


@needs_ref
@pytest.mark.parametrize("group", sorted(SAO_GROUPS))
@pytest.mark.parametrize("depth", [8, 10])
def test_sao_oracle_vs_reference(depth, group):
    R = T.load_ref(depth)
    for c, want in zip(sao_cases(depth, group), sao_oracle(depth, group)):
        got = T.sao_run_host(R, c)
        _same_stats(got, want, _name(c))
        _same_planes(got[2], want[2], (_name(c), "apply"))


# ---------------------------------------------------------------- level 2: the digest, and what the fixtures reach ----------------------------------------------------------------
@pytest.mark.parametrize("group", DB_GROUPS + tuple(sorted(SAO_GROUPS)))
@pytest.mark.parametrize("depth", [8, 10])
def test_oracle_matches_golden(depth, group):
    res = db_oracle(depth, group) if group.startswith("deblock") else sao_oracle(depth, group)
    assert digest(group, res) == _gold()[group][str(depth)]
    for c, r in zip([c for c, _ in db_cases(depth, group)] if group.startswith("deblock") else sao_cases(depth, group), res):
        for planes in (r if group.startswith("deblock") else [r[2]]):
            T.edge_margins_intact(depth, planes, c["width"], c["height"], _name(c))


@pytest.mark.parametrize("depth", [8, 10])
def test_deblock_strength_table(depth):
    """the oracle changes exactly the edges the table gives a strength above 0, in both directions"""
    (c, passes), = db_cases(depth, "deblock_strength")
    after = db_oracle(depth, "deblock_strength")[0][passes.index(3)]
    changed = T.deblock_strength_changed(c, c["planes"], after)
    seen = set()
    for (what, d, x, y, bs), ch in zip(c["edges"], changed):
        assert ch == (bs > 0), "%s, %s edge of the slot at x %d y %d: strength %d, samples %s" % (what, "horizontal" if d else "vertical", x, y, bs, "changed" if ch else "unchanged")
        seen.add((d, bs))
    assert seen == {(d, bs) for d in (0, 1) for bs in (0, 1, 2)}
    # strength 2 filters chroma, strength 1 does not: the table's edges lie off the chroma grid, the slots' borders next to an intra unit on it
    assert any((after[k] != c["planes"][k]).any() for k in (1, 2))


@pytest.mark.parametrize("depth", [8, 10])
def test_deblock_coverage(depth):
    pmax, scale = (1 << depth) - 1, 1 << (depth - 8)
    clips = {}
    ends = {(k, v): 0 for k in (0, 1) for v in (0, pmax)}
    strong = normal = 0
    for (c, passes), outs in zip(db_cases(depth, "deblock_params"), db_oracle(depth, "deblock_params")):
        for name, n in T.deblock_index_clips(c).items():
            clips[name] = clips.get(name, 0) + int(n)
        w, h = c["width"], c["height"]
        out = outs[passes.index(3)]
        for k in (0, 1, 2):
            a, b = T.edge_picture(c["planes"], w, h, k), T.edge_picture(out, w, h, k)
            for v in (0, pmax):
                ends[(min(k, 1), v)] += int(((b == v) & (a != v)).sum())
        # the vertical edges alone: only the strong filter writes the third sample from an edge (columns 5 and 2 of an 8x8 block); a changed edge whose step is at least
        # (5 * 24 + 1) / 2 << (depth - 8) cannot have passed the strong filter's last condition, whatever its tc
        a, b = T.edge_picture(c["planes"], w, h, 0).astype(np.int64), T.edge_picture(outs[passes.index(1)], w, h, 0).astype(np.int64)
        strong += int((a[:, 5::8] != b[:, 5::8]).sum()) + int((a[:, 2::8] != b[:, 2::8]).sum())
        m3, m4 = slice(7, w - 1, 8), slice(8, w, 8)
        normal += int(((np.abs(a[:, m3] - a[:, m4]) >= 61 * scale) & ((a[:, m3] != b[:, m3]) | (a[:, m4] != b[:, m4]))).sum())
    print("deblock coverage depth %d: index clips %s, samples newly at the range ends (plane kind, value) %s, strong %d, normal %d" % (depth, clips, ends, strong, normal))
    assert all(v > 0 for v in clips.values()), clips
    assert all(v > 0 for v in ends.values()), ends
    assert strong > 0 and normal > 0, (strong, normal)
    assert {k["offsets"][0] for k in DB_PARAMS} >= {-6, 0, 6} and {k["offsets"][1] for k in DB_PARAMS} >= {-6, 0, 6}
    assert {k["offsets"][2] for k in DB_PARAMS} >= {-12, 0, 12} and {k["offsets"][3] for k in DB_PARAMS} >= {-12, 0, 12}
    assert {(k["slice_b"], k["bypass"]) for k in DB_PARAMS} == {(a, b) for a in (False, True) for b in (False, True)}
    qps = np.concatenate([c["units"]["qp"] for c, _ in db_cases(depth, "deblock_params")])
    assert qps.min() == 0 and qps.max() == 51


@pytest.mark.parametrize("depth", [8, 10])
def test_sao_coverage(depth):
    top = 7 if depth == 8 else 31
    n = dict(clip_lo=0, clip_hi=0, wrapped=0)
    types = [set(), set()]
    for c in sao_cases(depth, "sao_params"):
        for k, v in T.sao_apply_coverage(c).items():
            n[k] += v
        p = c["params"]
        types[0] |= set(p["type"][:, 0].tolist()); types[1] |= set(p["type"][:, 1].tolist())
        assert p["offset"].min() == -top and p["offset"].max() == top
        assert (p["bandPos"][:, 1] != p["bandPos"][:, 2]).any() and (p["offset"][:, 1] != p["offset"][:, 2]).any()
    print("SAO coverage depth %d: %s" % (depth, n))
    assert all(v > 0 for v in n.values()), n
    assert types[0] == types[1] == set(range(-1, 5))
    assert any(t0 != t1 for c in sao_cases(depth, "sao_params") for t0, t1 in c["params"]["type"].tolist())
    assert {int(b) for c in sao_cases(depth, "sao_params") for b in c["params"]["bandPos"].ravel()} >= {28, 29, 30, 31}
    # the statistics over all SAO cases
    total = np.zeros((3, 5, 32), np.int64)
    for group in SAO_GROUPS:
        for cnt, org, _ in sao_oracle(depth, group):
            total += cnt.reshape(-1, 3, 5, 32).sum(0)
    for plane in range(3):
        assert (total[plane, :4, :5] > 0).all(), ("an edge class without samples", plane, total[plane, :4, :5])
        assert total[plane, 4, 0] > 0 and total[plane, 4, 31] > 0, ("first / last band without samples", plane)
    # flat: class 0 alone; checkerboard: along x and y local minima and maxima alone, along the diagonals (whose neighbours equal the sample) class 0 alone
    for c, (cnt, org, _) in zip(sao_cases(depth, "sao_stats"), sao_oracle(depth, "sao_stats")):
        e = cnt.reshape(-1, 3, 5, 32)[:, :, :4, :5].sum((0, 1))             # [type][class]
        if c["content"] == "flat":
            assert (e[:, 0] > 0).all() and not e[:, 1:].any(), e
        if c["content"] == "checker":
            assert (e[:2, [1, 4]] > 0).all() and not e[:2, [0, 2, 3]].any() and (e[2:, 0] > 0).all() and not e[2:, 1:].any(), e
        if c["content"] == "saturated":
            assert np.abs(org).max() > 60 * ((1 << depth) - 8), ("the sums hold no large differences", int(np.abs(org).max()))


# ---------------------------------------------------------------- level 3: the kernels against the oracle ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("group", DB_GROUPS)
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_deblock_edges(depth, group):
    H = T.load_hip(depth)
    res = []
    for (c, passes), wants in zip(db_cases(depth, group), db_oracle(depth, group)):
        per = []
        for p, want in zip(passes, wants):
            forms = T.deblock_run_hip_forms(H, c, p)
            for form, got in forms.items():
                _same_planes(got, want, (_name(c), "passes %d" % p, form))         # margins included: nothing outside the picture written
            per.append(forms["picture"])
        res.append(per)
    assert digest(group, res) == _gold()[group][str(depth)]


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(SAO_GROUPS))
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_sao_edges(depth, group):
    H = T.load_hip(depth)
    res = []
    for c, want in zip(sao_cases(depth, group), sao_oracle(depth, group)):
        forms = T.sao_run_hip_forms(H, c)
        for form, (cnt, org, out, rec) in forms.items():
            _same_stats((cnt, org), want, (_name(c), form))
            _same_planes(rec, c["rec"], (_name(c), form, "the deblocked input"))
            _same_planes(out, want[2] if form != "odd" else c["rec"], (_name(c), form, "apply"))
        res.append(forms["picture"][:3])
    assert digest(group, res) == _gold()[group][str(depth)]
