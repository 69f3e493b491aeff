"""The view-overlap closed form (include/vicasplat_overlap.h) and the evaluation-index generator on the CPU: the float64 restatement of
tests/overlap_f64.py and the torch backend against the real reference's counts in tests/golden/view_overlap.npz, planted defects, the
generator against the reference's index, the binding of vso_view_overlap_counts and its refusals, get_overlap_tag.

Measured here (`-s` prints them): r32 per compared quantity at most 0.77 units; the largest ambiguous share of a case's ray-pairs;
the rays each planted defect moves beyond the ambiguity.  The case `edge` is exact in f32 only (its c_y IS the f32 bound, which is another
number than the f64 bound): every ray of it is ambiguous for the restatement by construction, so it is held to the reference's own f32
counts bit for bit (test_exact_edge_in_f32) and takes no part in the ambiguity cap.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import overlap_f64 as O

G = O.golden()
AMBIGUOUS_CAP = 0.005


CASES = O.cases(G)
BAND_CASES = [c for c in CASES if c[0] != "edge"]


def test_builders_give_the_cameras_of_the_golden():
    E, K = O.trajectory()
    sE, sK, named = O.special()
    assert np.array_equal(E, G["traj_E"]) and np.array_equal(K, G["traj_K"])
    assert np.array_equal(sE, G["spec_E"], equal_nan=True) and np.array_equal(sK, G["spec_K"])
    assert [tuple(p) for p in G["spec_pairs"]] == [p for n in named for p in named[n]]


@pytest.mark.parametrize("case", BAND_CASES, ids=[c[0] for c in BAND_CASES])
def test_restatement_and_torch_backend_against_the_reference(case):
    from vicasplat_amd.geometry.epipolar_lines import view_overlap_counts
    name, E, K, pairs, key, sl = case
    rays = ambiguous = ref_gap = 0
    for h, w in O.SIZES:
        ref32, ref64 = G[f"{key}_ref32_{h}x{w}"][sl], G[f"{key}_ref64_{h}x{w}"][sl]
        count, sure, amb = O.counts(E, K, h, w, pairs)
        assert np.array_equal(count, ref64), (name, h, w)          # the closed form IS what the reference computes
        assert ((ref32 >= sure) & (ref32 <= sure + amb)).all(), (name, h, w)
        prs = torch.tensor(pairs)
        t64 = view_overlap_counts(torch.tensor(E), torch.tensor(K), (h, w), prs, backend="torch").numpy()
        t32 = view_overlap_counts(torch.tensor(E).float(), torch.tensor(K).float(), (h, w), prs, backend="torch").numpy()
        assert np.array_equal(t64, ref64) and ((t32 >= sure) & (t32 <= sure + amb)).all(), (name, h, w)
        rays, ambiguous, ref_gap = rays + h * w * len(pairs), ambiguous + int(amb.sum()), max(ref_gap, int(np.abs(ref32 - ref64).max()))
    print(f"{name}: ambiguous share {ambiguous / rays:.2e}, reference f32 - f64 at most {ref_gap} rays")
    assert ambiguous / rays <= AMBIGUOUS_CAP and ref_gap <= max(1, int(AMBIGUOUS_CAP * 32 * 48))


def test_r32_is_measured():
    """The restatement's own f32 - f64 gap of every compared quantity, in units of 2^-24 mag, over the case list: not above overlap_f64.R32."""
    worst = {}
    for name, E, K, pairs, _, _ in CASES:
        if name == "nan":
            continue
        for h, w in ((16, 16), (17, 23)):
            for i, j in pairs[:: max(1, len(pairs) // 24)]:
                r32, r64 = {}, {}
                O.flags(E, K, h, w, i, j, np.float32, record=r32)
                O.flags(E, K, h, w, i, j, np.float64, record=r64)
                for k in r64:
                    with np.errstate(all="ignore"):
                        gap = np.abs(r32[k].v.astype(np.float64) - r64[k].v) / (O.U * r64[k].e)
                    gap = gap[np.isfinite(gap) & np.isfinite(r64[k].e)]
                    q = k.rstrip("0123").replace("_x", "").replace("_y", "")
                    worst[q] = max(worst.get(q, 0.0), float(gap.max()) if gap.size else 0.0)
    print("r32:", {k: round(v, 3) for k, v in worst.items()})
    for q, v in worst.items():
        assert v <= O.R32[q], (q, v)


def test_planted_defects_move_a_golden_count():
    """Every planted defect moves a count of the golden by at least one ray beyond the ambiguity.  The case `edge` is run in f32 against the
    reference's f32 counts (the bound it sits on is the f32 one); every other case in f64 against its f64 counts."""
    moved = dict.fromkeys(O.MUTANTS, 0)
    for name, E, K, pairs, key, sl in CASES:
        if name == "nan":
            continue
        for h, w in (((16, 16), (17, 23)) if name == "trajectory" else O.SIZES):
            if name == "edge":
                ref = G[f"{key}_ref32_{h}x{w}"][sl]
                base, _, _ = O.counts(E, K, h, w, pairs, np.float32)
                assert np.array_equal(base, ref), (h, w)
                got, _, _ = O.counts(E, K, h, w, pairs, np.float32, mutant="strict_bounds")
                moved["strict_bounds"] = max(moved["strict_bounds"], int(np.abs(got - ref).max()))
                continue
            ref = G[f"{key}_ref64_{h}x{w}"][sl]
            _, sure, amb = O.counts(E, K, h, w, pairs)
            for m in O.MUTANTS:
                got, _, _ = O.counts(E, K, h, w, pairs, mutant=m)
                beyond = np.maximum(got - (sure + amb), sure - got)
                moved[m] = max(moved[m], int(beyond.max()), int(np.abs(got - ref).max() - amb.max()))
    print("planted defects, rays beyond the ambiguity:", moved)
    for m in O.MUTANTS:
        assert moved[m] >= 1, m


def test_exact_edge_in_f32():
    """`other` of the frame line x = 1 equals the f32 bound exactly (-f32(1e-6), f32(1 + 1e-6)): `>=` and `<=` keep the ray, as the reference's
    f32 run does; the strict comparisons lose it.  The restatement and the torch backend in f32, bit for bit."""
    from vicasplat_amd.geometry.epipolar_lines import view_overlap_counts
    name, E, K, pairs, key, sl = next(c for c in CASES if c[0] == "edge")
    for h, w in O.SIZES:
        ref32 = G[f"{key}_ref32_{h}x{w}"][sl]
        count, _, _ = O.counts(E, K, h, w, pairs, np.float32)
        t32 = view_overlap_counts(torch.tensor(E).float(), torch.tensor(K).float(), (h, w), torch.tensor(pairs), backend="torch").numpy()
        assert np.array_equal(count, ref32) and np.array_equal(t32, ref32), (h, w, count, t32, ref32)
    strict, _, _ = O.counts(E, K, 1, 1, pairs, np.float32, mutant="strict_bounds")
    assert G[f"{key}_ref32_1x1"][sl].tolist() == [1, 1] and strict.tolist() == [0, 0]


def test_generator_reproduces_the_reference_index(tmp_path):
    from vicasplat_amd.evaluation import IndexEntry
    gen, text = O.run_generator(G, tmp_path, "torch", "cpu")
    assert text == str(G["index_json"])
    want = json.loads(text)
    assert list(gen.index) == list(want) and '"overlap": null' in text and gen.index["none"] is None
    assert gen.index["first"] == IndexEntry(tuple(want["first"]["context"]), tuple(want["first"]["target"]))
    assert G["scene_starts"].tolist()[1] > 1 and G["scene_starts"].tolist()[2] == O.SCENE_V and G["scene_randints"].tolist()[3] > 2


def test_save_previews_raises(tmp_path):
    from vicasplat_amd.evaluation import EvaluationIndexGenerator, EvaluationIndexGeneratorCfg
    with pytest.raises(NotImplementedError, match="save_previews"):
        EvaluationIndexGenerator(EvaluationIndexGeneratorCfg(output_path=tmp_path, **dict(O.SCENE_CFG, save_previews=True)))


def test_entry_is_bound_from_the_eighth_header_and_checks_its_arguments():
    from vicasplat_amd import _lib
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    sigs = _lib.parse_header(open(os.path.join(inc, "vicasplat_overlap.h")).read(), prefix="vso_")
    assert set(sigs) == {"vso_view_overlap_counts"}
    restype, argtypes, takes_stream = sigs["vso_view_overlap_counts"]
    i32, vp = C.c_int32, C.c_void_p
    assert restype is C.c_int and argtypes == [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp] and takes_stream
    L = _lib.lib()
    p, f, err = C.c_void_p(16), L.vso_view_overlap_counts, L.vs_last_error
    # every refusal comes before any HIP call: there is no device here
    for k in (0, 1, 6, 8):
        args = [p, p, 0, 2, 4, 4, p, 1, p]
        args[k] = None
        assert f(*args, None) < 0 and b"vso_view_overlap_counts: null pointer" in err()
    for code in (1, 2, 3, 4, 6, -1):
        assert f(p, p, code, 2, 4, 4, p, 1, p, None) < 0 and b"dtype %d" % code in err()
    assert f(p, p, 0, 0, 4, 4, p, 1, p, None) < 0 and b"V = 0" in err()
    assert f(p, p, 0, 2, 0, 4, p, 1, p, None) < 0 and b"H = 0" in err()
    assert f(p, p, 0, 2, 4, 0, p, 1, p, None) < 0 and b"W = 0" in err()
    assert f(p, p, 0, 2, 4, 4, p, -1, p, None) < 0 and b"P = -1" in err()
    assert f(p, p, 0, 2, 1 << 15, (1 << 15) + 1, p, 1, p, None) < 0 and b"exceed 2^30" in err()
    assert f(None, None, 5, 2, 4, 4, None, 0, None, None) == 0          # P = 0: nothing to do, nothing launched


def test_wrappers_refuse_what_they_cannot_take():
    from vicasplat_amd.geometry.epipolar_lines import view_overlap, view_overlap_counts
    E, K, prs = torch.eye(4).repeat(3, 1, 1), torch.eye(3).repeat(3, 1, 1), torch.tensor([[0, 1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        view_overlap_counts(E, K, (4, 4), prs, backend="hip")
    with pytest.raises(ValueError, match="backend"):
        view_overlap_counts(E, K, (4, 4), prs, backend="cuda")
    with pytest.raises(ValueError, match="one dtype"):
        view_overlap_counts(E, K.double(), (4, 4), prs)
    with pytest.raises(ValueError, match="f32 or f64"):
        view_overlap_counts(E.half(), K.half(), (4, 4), prs)
    with pytest.raises(ValueError, match=r"\[P, 2\]"):
        view_overlap_counts(E, K, (4, 4), prs[0])
    with pytest.raises(ValueError, match="image shape"):
        view_overlap_counts(E, K, (0, 4), prs)
    out = view_overlap(E, K, (4, 4), torch.tensor([[0, 0], [0, 7]]))
    assert out.dtype == torch.float32 and out[0] == 1.0 and out[1] < 0
    assert view_overlap_counts(E, K, (4, 4), prs[:0]).shape == (0,)
    # counts / N as torch's own mean gives it on the CPU
    flags = torch.arange(391)[None] < torch.tensor([0, 1, 130, 390, 391])[:, None]
    from vicasplat_amd.geometry.epipolar_lines import overlap_from_counts
    assert torch.equal(overlap_from_counts(flags.sum(1).int(), 391), torch.stack([f.float().mean() for f in flags]))


def test_get_overlap_tag_at_its_boundaries():
    from vicasplat_amd.misc.utils import get_overlap_tag
    assert [get_overlap_tag(v) for v in (0.05, 0.3, 0.3000001, 0.55, 0.5500001, 0.8, 0.8000001)] == \
        ["small", "small", "medium", "medium", "large", "large", "ignore"]
    assert get_overlap_tag(0.0499) == "medium" and get_overlap_tag(1.0) == "ignore"      # below 0.05 falls through, as in the reference
