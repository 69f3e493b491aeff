"""The data shims on the CPU: the numpy restatement of tests/data_shims_ref.py against the installed PIL (0 differing bytes) and against the
golden vectors of the real reference (tests/golden/crop_shim.npz), the package's coefficient tables against the restatement's, the package's
Python parts that need no GPU (intrinsics, extrinsics reflection, the augmentation draw) against the golden, the planted defects, the sixth
header and the argument checks of vsp_rescale_crop, and the float quantisation rule.  The kernel itself: tests/test_data_shims_gpu.py.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import data_shims_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "crop_shim.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---- 1. the restatement against the installed PIL ----
@pytest.mark.parametrize("src,dst", R.PIL_SHAPES, ids=[f"{s[0]}x{s[1]}" for s, _ in R.PIL_SHAPES])
def test_restatement_equals_pil(src, dst):
    from PIL import Image
    (h_in, w_in), (h, w) = src, dst
    for fill in R.FILLS:
        frame = R.make_frames(1, h_in, w_in, fill, seed=3)[0]
        for mirror in (False, True):
            img = np.ascontiguousarray(frame[:, ::-1]) if mirror else frame
            want = np.array(Image.fromarray(img).resize((w, h), Image.LANCZOS))
            got = R.resize(img, h, w)
            differing = int((got != want).sum())
            print(f"{h_in}x{w_in} -> {h}x{w} {fill} mirror={mirror}: {differing} differing bytes")
            assert got.shape == want.shape and differing == 0
            if fill == "constant":
                assert (got == 255).all()
            if fill == "extremes":
                assert got.min() == 0 and got.max() == 255      # both clamps act: the filter over- and undershoots on 0 / 255 edges


def test_tap_counts_of_the_named_shapes():
    assert R.coeffs(960, 341)[1].shape[1] == 19 and R.coeffs(960, 455)[1].shape[1] == 15 and R.coeffs(640, 455)[1].shape[1] == 11
    worst = max(np.abs(R.coeffs(a, b)[1].astype(np.int64)).sum(1).max() for (h0, w0), (h1, w1) in R.PIL_SHAPES for a, b in ((h0, h1), (w0, w1)) if a != b)
    print("largest sum|k| / 2^22:", worst / (1 << 22))
    assert 255 * int(worst) + (1 << 21) < 1 << 31


# ---- 2. the package's tables ----
def test_package_tables_equal_the_restatement():
    from vicasplat_amd.dataset.shims import crop_shim
    pairs = {(a, b) for (h0, w0), (h1, w1) in R.PIL_SHAPES for a, b in ((h0, h1), (w0, w1)) if a != b} | {(80, 32), (71, 31), (50, 33)}
    for n_in, n_out in sorted(pairs):
        bounds, k = crop_shim.resample_tables(n_in, n_out)
        ref_bounds, ref_k = R.coeffs(n_in, n_out)
        assert bounds.dtype == k.dtype == np.int32 and np.array_equal(bounds, ref_bounds) and np.array_equal(k, ref_k), (n_in, n_out)
        assert crop_shim.resample_tables(n_in, n_out)[1] is k          # cached
    with pytest.raises(ValueError, match="reductions"):
        crop_shim.resample_tables(10, 11)
    with pytest.raises(ValueError, match="taps"):
        crop_shim.resample_tables(4000, 100)


def test_overflow_guard_raises_on_a_made_up_table():
    from vicasplat_amd.dataset.shims import crop_shim
    ok = np.full((2, 11), (1 << 22) // 8, np.int32)          # sum|k| = 1.375 x 2^22
    crop_shim.check_overflow(ok)
    bad = ok.copy()
    bad[1, ::2] = -(1 << 22)          # sum|k| > 2 x 2^22: 255 sum|k| passes 2^31
    with pytest.raises(OverflowError, match="int32"):
        crop_shim.check_overflow(bad)


# ---- 3. the golden of the real reference ----
def test_restatement_reproduces_the_golden(golden):
    for ex_name in R.GOLDEN_EXAMPLES:
        ex = R.golden_example(ex_name)
        assert R.example_digest(ex) == str(golden[f"{ex_name}_sha256"])
        for form in ("plain", "reflected"):
            for g in ("context", "target"):
                got = R.shim_views(ex[g], R.GOLDEN_SHAPE, mirror=form == "reflected")
                key = f"{ex_name}_{form}_{g}"
                want_u8 = golden[key + "_image_u8"]
                assert np.array_equal(np.moveaxis(got["image_u8"], -1, 1), want_u8), key
                assert np.array_equal(got["image"], want_u8.astype(np.float32) / np.float32(255)), key
                assert np.array_equal(got["intrinsics"], golden[key + "_intrinsics"]), key
                assert np.array_equal(got["extrinsics"], golden[key + "_extrinsics"]), key
    h, w, _ = R.GOLDEN_EXAMPLES["wide"]
    assert R.scaled_size(h, w, R.GOLDEN_SHAPE) == (32, 57) and R.crop_frame(np.zeros((h, w, 3), np.uint8), R.GOLDEN_SHAPE)[1] == (0, 12)
    h, w, _ = R.GOLDEN_EXAMPLES["tall"]
    assert R.scaled_size(h, w, R.GOLDEN_SHAPE) == (57, 32) and R.crop_frame(np.zeros((h, w, 3), np.uint8), R.GOLDEN_SHAPE)[1] == (12, 0)


def test_package_python_parts_reproduce_the_golden(golden):
    from vicasplat_amd.dataset.shims import augmentation_shim, crop_shim
    for ex_name, (h, w, _) in R.GOLDEN_EXAMPLES.items():
        ex = R.golden_example(ex_name)
        h_scaled, w_scaled = crop_shim.scaled_size(h, w, R.GOLDEN_SHAPE)
        assert (h_scaled, w_scaled) == R.scaled_size(h, w, R.GOLDEN_SHAPE)
        for g in ("context", "target"):
            K, E = torch.tensor(ex[g]["intrinsics"]), torch.tensor(ex[g]["extrinsics"])
            scaled = torch.zeros(K.shape[0], 3, h_scaled, w_scaled)
            window, K2 = crop_shim.center_crop(scaled, K, R.GOLDEN_SHAPE)
            assert tuple(window.shape[-2:]) == R.GOLDEN_SHAPE and np.array_equal(K2.numpy(), golden[f"{ex_name}_plain_{g}_intrinsics"])
            assert np.array_equal(K.numpy(), ex[g]["intrinsics"])          # the input is not modified
            assert np.array_equal(augmentation_shim.reflect_extrinsics(E).numpy(), golden[f"{ex_name}_reflected_{g}_extrinsics"])
            views = augmentation_shim.reflect_views(dict(image=torch.tensor(ex[g]["image"]), extrinsics=E, intrinsics=K))
            assert views[crop_shim.MIRROR_KEY].tolist() == [1] * K.shape[0] and views["image"].shape == ex[g]["image"].shape
            assert augmentation_shim.reflect_views(views)[crop_shim.MIRROR_KEY].tolist() == [0] * K.shape[0]
    with pytest.raises(AssertionError):
        crop_shim.scaled_size(30, 80, (32, 32))          # the reference's assertion: h_out <= h_in
    # the draw: the reference's decisions for the first 16 draws of a generator seeded with 0
    gen = torch.Generator().manual_seed(0)
    token = dict(context=dict(image=torch.zeros(1, 3, 2, 2), extrinsics=torch.eye(4)[None]), target=dict(image=torch.zeros(1, 3, 2, 2), extrinsics=torch.eye(4)[None]))
    unchanged = []
    for _ in range(16):
        out = augmentation_shim.apply_augmentation_shim(token, gen)
        unchanged.append(out is token)
        if out is not token:
            assert crop_shim.MIRROR_KEY in out["context"] and crop_shim.MIRROR_KEY in out["target"] and float(out["context"]["extrinsics"][0, 0, 0]) == 1.0
    assert unchanged == golden["augmentation_unchanged"].tolist() and 0 < sum(unchanged) < 16


def test_crop_shim_refuses_cpu_tensors():
    from vicasplat_amd.dataset.shims import crop_shim
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crop_shim.rescale(torch.zeros(3, 8, 8), (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crop_shim.apply_crop_shim_to_views(dict(image=torch.zeros(2, 3, 8, 8, dtype=torch.uint8), intrinsics=torch.eye(3).repeat(2, 1, 1)), (4, 4))


# ---- 4. planted defects ----
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_planted_defect_changes_the_golden_example(golden, mutant):
    """Each defect changes at least one byte (for div_256: one float) of the reflected 45 x 80 example, whose crop difference is odd."""
    ex = R.golden_example("wide")
    changed = 0
    for g in ("context", "target"):
        got = R.shim_views(ex[g], R.GOLDEN_SHAPE, mirror=True, mutant=mutant)
        want_u8 = golden[f"wide_reflected_{g}_image_u8"]
        if mutant == "div_256":
            changed += int((got["image"] != want_u8.astype(np.float32) / np.float32(255)).sum())
        else:
            changed += int((np.moveaxis(got["image_u8"], -1, 1) != want_u8).sum())
    print(f"{mutant}: {changed} elements differ from the golden")
    assert changed >= 1


# ---- 5. the sixth header ----
def test_entry_is_bound_from_the_sixth_header_and_checks_its_arguments():
    from vicasplat_amd import _lib
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    sigs = _lib.parse_header(open(os.path.join(inc, "vicasplat_data.h")).read(), prefix="vsp_")
    assert set(sigs) == {"vsp_rescale_crop"}
    restype, argtypes, takes_stream = sigs["vsp_rescale_crop"]
    i32, vp = C.c_int32, C.c_void_p
    assert restype is C.c_int and takes_stream
    assert argtypes == [vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L = _lib.lib()
    p = C.c_void_p(16)
    three = (C.c_float * 3)(0.5, 0.5, 0.5)
    err = lambda: L.vs_last_error()

    def call(src=p, layout=0, N=1, h_in=45, w_in=80, bx=p, kx_t=p, w_scaled=57, kx=11, by=p, ky_t=p, h_scaled=32, ky=11, row=0, col=12, h_out=32,
             w_out=32, mirror=None, mean=None, std=None, out=p):
        return L.vsp_rescale_crop(src, layout, N, h_in, w_in, bx, kx_t, w_scaled, kx, by, ky_t, h_scaled, ky, row, col, h_out, w_out, mirror, mean, std,
                                  out, None)
    # every refusal comes before any HIP call: there is no device here
    assert call(src=None) < 0 and b"vsp_rescale_crop: null pointer" in err()
    assert call(out=None) < 0 and b"null pointer" in err()
    assert call(layout=3) < 0 and b"layout 3" in err()
    assert call(layout=-1) < 0 and b"layout -1" in err()
    assert call(N=-1) < 0 and b"N = -1" in err()
    assert call(h_in=0) < 0 and b"at least 1" in err()
    assert call(w_out=0) < 0 and b"at least 1" in err()
    assert call(h_out=-3) < 0 and b"at least 1" in err()
    assert call(w_scaled=81) < 0 and b"enlarging" in err()
    assert call(h_scaled=46) < 0 and b"enlarging" in err()
    assert call(col=26) < 0 and b"crop window" in err()          # 26 + 32 > 57
    assert call(row=1) < 0 and b"crop window" in err()
    assert call(col=-1) < 0 and b"crop window" in err()
    assert call(h_out=33) < 0 and b"crop window" in err()
    assert call(bx=None) < 0 and b"null horizontal table" in err()
    assert call(ky_t=None) < 0 and b"null vertical table" in err()
    assert call(kx=129) < 0 and b"kx = 129" in err()
    assert call(ky=0) < 0 and b"ky = 0" in err()
    assert call(mean=three) < 0 and b"mean and std" in err()
    assert call(std=three) < 0 and b"mean and std" in err()
    assert call(N=0) == 0 and call(N=0, mean=three, std=three) == 0          # N = 0: nothing to do, nothing launched
    # a skipped pass needs no table: the refusals above do not apply, N = 0 ends the call
    assert call(N=0, w_in=57, bx=None, kx_t=None, kx=0) == 0 and call(N=0, h_in=32, by=None, ky_t=None, ky=0) == 0


# ---- 6. the float quantisation rule ----
def test_float_quantisation_rule_matches_the_torch_expression():
    u = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal((np.arange(256) / 255).astype(np.float32), u)          # the reference's float64 division cast to f32
    below, above = np.nextafter(u, np.float32(-np.inf)), np.nextafter(u, np.float32(np.inf))
    outside = np.array([-1.0, -1e-3, -0.0, -1e-45, 1.0 + 1e-6, 1.5, 300.0, np.inf, -np.inf], np.float32)
    g = np.random.default_rng(0)
    x = np.concatenate([u, below, above, outside, g.uniform(-0.1, 1.1, 4096).astype(np.float32)])
    want = (torch.tensor(x) * 255).clip(min=0, max=255).type(torch.uint8).numpy()
    got = R.quantise(x)
    assert np.array_equal(got, want)
    assert np.array_equal(R.quantise(u), np.arange(256, dtype=np.uint8))          # exact u / 255 comes back as u
    assert (R.quantise(below[1:]) == np.arange(255, dtype=np.uint8)).all() and R.quantise(np.array([np.nan], np.float32))[0] == 0
