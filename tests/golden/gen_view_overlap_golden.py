"""Generates tests/golden/view_overlap.npz from the real reference, imported on the CPU through ref_import.py: the counts of its own
project_rays / get_world_rays / sample_image_grid on the cameras of tests/overlap_f64.py, in f32 and in f64, and the index that its own
EvaluationIndexGenerator writes for five seeded scenes (Lightning is a stub, so the instance's `device` is set to the CPU by hand).

Keys
  traj_E [16, 4, 4], traj_K [16, 3, 3] f64 (every entry an f32 value): overlap_f64.trajectory(); traj_ref32_<h>x<w>, traj_ref64_<h>x<w>
  [256] int32: the reference's counts of all ordered pairs (i, j) = divmod(p, 16) with f32 and with f64 cameras, for the sizes of
  overlap_f64.SIZES.  spec_E, spec_K, spec_pairs [P, 2], spec_ref32_<h>x<w>, spec_ref64_<h>x<w>: the same for overlap_f64.special(), its
  pairs in the order of its dictionary.
  scene_names, scene_seeds, scene_E [5, 24, 4, 4], scene_K: the five scenes; index_json: the evaluation_index.json the reference wrote;
  scene_starts: the start frames it tried per scene; scene_randints: its torch.randint calls per scene; cfg_seed: the generator's seed
  (searched upwards from overlap_f64.SCENE_CFG's).
At generation time every scene is checked to be the kind its name says, and every overlap the reference's control flow compares to lie at
least (ambiguous rays + 1) / N away from min_overlap and from max_overlap (ambiguous rays: the most of any pair of the scene's band):
otherwise the golden would pin rounding.  Seeds are searched from 0 up.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_view_overlap_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main() -> None:
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import ref_import
    ref_import.install()
    import src.evaluation.evaluation_index_generator as ref_gen
    from src.geometry.epipolar_lines import project_rays
    from src.geometry.projection import get_world_rays, sample_image_grid
    from einops import rearrange
    import overlap_f64 as O
    from vicasplat_amd.evaluation import band_pairs

    def ref_counts(E, K, h, w, pairs, dtype):
        E, K = torch.tensor(E, dtype=dtype), torch.tensor(K, dtype=dtype)
        xy = rearrange(sample_image_grid((h, w))[0], "h w xy -> (h w) xy").to(dtype)
        out = []
        for i, j in pairs:
            origins, directions = get_world_rays(xy, E[i], K[i])
            out.append(int(project_rays(origins, directions, E[j], K[j])["overlaps_image"].sum()))
        return np.array(out, np.int32)

    out = dict(torch_version=np.array(torch.__version__))
    E, K = O.trajectory()
    sE, sK, spairs = O.special()
    flat = [p for name in spairs for p in spairs[name]]
    out.update(traj_E=E, traj_K=K, spec_E=sE, spec_K=sK, spec_pairs=np.array(flat, np.int32))
    for h, w in O.SIZES:
        for tag, dtype in (("ref32", torch.float32), ("ref64", torch.float64)):
            out[f"traj_{tag}_{h}x{w}"] = ref_counts(E, K, h, w, O.all_pairs(16), dtype)
            out[f"spec_{tag}_{h}x{w}"] = ref_counts(sE, sK, h, w, flat, dtype)
        print((h, w), "f32 != f64 on", int((out[f"traj_ref32_{h}x{w}"] != out[f"traj_ref64_{h}x{w}"]).sum()), "trajectory pairs")

    # ---- the evaluation index of five scenes, one generator over all of them (one seed, as the reference runs it)
    h, w = O.SCENE_SHAPE
    N, cfgd = h * w, dict(O.SCENE_CFG)
    names = ["first", "later", "none", "repeat", "max_distance"]
    band = band_pairs(O.SCENE_V, cfgd["min_distance"], cfgd["max_distance"]).numpy()

    def margin(E, K):
        """(the most ambiguous rays of a pair of the scene's band + 1) / N"""
        return (int(O.counts(E, K, h, w, band)[2].max()) + 1) / N

    starts, randints, compared = [], [], []
    real_tqdm, real_randint, real_project = ref_gen.tqdm, torch.randint, ref_gen.project_rays

    def tqdm(it, *a, **k):
        for x in it:
            starts[-1] += 1
            yield x

    def randint(*a, **k):
        randints[-1] += 1
        return real_randint(*a, **k)

    def project(*a, **k):
        r = real_project(*a, **k)
        compared[-1].append(float(r["overlaps_image"].float().mean()))
        return r

    def run(seeds):
        with tempfile.TemporaryDirectory() as tmp:
            gen = ref_gen.EvaluationIndexGenerator(ref_gen.EvaluationIndexGeneratorCfg(output_path=Path(tmp), **cfgd))
            gen.device = torch.device("cpu")
            del starts[:], randints[:], compared[:]
            ref_gen.tqdm, torch.randint, ref_gen.project_rays = tqdm, randint, project
            try:
                for name, seed in zip(names, seeds):
                    E, K = O.scene(name, seed)
                    starts.append(0), randints.append(0), compared.append([])
                    batch = dict(target=dict(image=torch.zeros(1, O.SCENE_V, 3, h, w), extrinsics=torch.tensor(E, dtype=torch.float32)[None],
                                             intrinsics=torch.tensor(K, dtype=torch.float32)[None]), scene=[name])
                    gen.test_step(batch, 0)
            finally:
                ref_gen.tqdm, torch.randint, ref_gen.project_rays = real_tqdm, real_randint, real_project
            gen.save_index()
            return dict(gen.index), (Path(tmp) / "evaluation_index.json").read_text()

    def failing(index, seeds):
        """The first scene that is not of its kind, or that compares an overlap too close to a bound; None when all five hold."""
        walk = cfgd["max_distance"] + 2 - cfgd["min_distance"]      # the comparisons of one whole walk in one direction
        pair_min = lambda c: [min(c[k], c[k + 1]) for k in range(0, len(c), 2)]
        kinds = [index["first"] is not None and starts[0] == 1,
                 index["later"] is not None and starts[1] > 1,
                 index["none"] is None and starts[2] == O.SCENE_V,
                 index["repeat"] is not None and randints[3] > 2,
                 index["max_distance"] is not None and min(pair_min(compared[4])) >= cfgd["min_overlap"] and len(compared[4]) // 2 >= walk]
        for k, name in enumerate(names):
            m = margin(*O.scene(name, seeds[k]))
            away = all(abs(v - bound) >= m for v in compared[k] for bound in (cfgd["min_overlap"], cfgd["max_overlap"]))
            if not (kinds[k] and away):
                return k
        return None

    # the first generator seed, and under it the first scene seeds, for which every scene is of its kind (the draws depend on the generator's
    # state, which a scene's own seed hardly moves: so the generator's seed is searched too)
    for cfg_seed in range(cfgd["seed"], cfgd["seed"] + 50):
        cfgd = dict(cfgd, seed=cfg_seed)
        seeds = [0] * 5
        for attempt in range(8):
            index, text = run(seeds)
            k = failing(index, seeds)
            if os.environ.get("GEN_DEBUG"):
                print(cfg_seed, seeds, starts, randints, [len(c) for c in compared], k)
            if k is None:
                break
            seeds[k] += 1
        if k is None:
            break
    else:
        raise SystemExit("no seeds found")
    print("seeds", seeds, "starts", starts, "randints", randints, "index", index)
    scenes = [O.scene(n, s) for n, s in zip(names, seeds)]
    out.update(scene_names=np.array(names), scene_seeds=np.array(seeds), scene_E=np.stack([s[0] for s in scenes]),
               scene_K=np.stack([s[1] for s in scenes]), index_json=np.array(text), scene_starts=np.array(starts),
               scene_randints=np.array(randints), cfg_seed=np.array(cfg_seed))
    path = os.path.join(HERE, "view_overlap.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
