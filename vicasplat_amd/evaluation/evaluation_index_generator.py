"""The evaluation-index generator of the reference's src/evaluation/evaluation_index_generator.py: the step that writes
`evaluation_index.json`, which the test runs read through ViewSamplerEvaluation.

The reference walks outwards from a start frame and, at every step, casts all h w rays of two cameras through `project_rays` twice and
ends in `.item()`.  Here `test_step` makes ONE `view_overlap_counts` call for both directions of every pair (a, b) with
min_distance <= |a - b| <= max_distance + 1 (the walk stops after the first frame beyond max_distance, so it looks no further), copies the
counts to the host once, and then runs the reference's control flow on the host, line for line: the same `torch.Generator` draws in the same
order (`randperm(v)`, the `randint` for the choice, the `randint` loop for distinct targets), the same stepping and stop rule, the same f32
comparison of count / N against the configured bounds, the same `for ... else` to `None`.
"""
from __future__ import annotations

import json
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Optional

import torch

from ..geometry.epipolar_lines import overlap_from_counts, view_overlap_counts


@dataclass
class EvaluationIndexGeneratorCfg:
    num_target_views: int
    min_distance: int
    max_distance: int
    min_overlap: float
    max_overlap: float
    output_path: Path
    save_previews: bool
    seed: int


@dataclass
class IndexEntry:
    context: tuple[int, ...]
    target: tuple[int, ...]
    overlap: Optional[str | float] = None  # choose from ["small", "medium", "large"] or a float number indicates the overlap ratio


def band_pairs(v: int, min_distance: int, max_distance: int) -> torch.Tensor:
    """pairs [P, 2] int32 on the CPU: (a, b) and (b, a) for every a < b < v with min_distance <= b - a <= max_distance + 1."""
    a = torch.arange(v, dtype=torch.int32)
    blocks = []
    for d in range(max(int(min_distance), 0), min(int(max_distance) + 1, v - 1) + 1):
        lo, hi = a[:v - d], a[:v - d] + d
        blocks += [torch.stack([lo, hi], -1), torch.stack([hi, lo], -1)]
    return torch.cat(blocks) if blocks else torch.zeros(0, 2, dtype=torch.int32)


class EvaluationIndexGenerator:
    """A plain class with the reference's `test_step(batch, batch_idx)`, `save_index()` and `index`.  backend: that of
    view_overlap_counts (None: "hip" for device tensors)."""
    generator: torch.Generator
    cfg: EvaluationIndexGeneratorCfg
    index: dict[str, IndexEntry | None]

    def __init__(self, cfg: EvaluationIndexGeneratorCfg, backend: str | None = None) -> None:
        if cfg.save_previews:
            raise NotImplementedError("EvaluationIndexGenerator: save_previews=True needs add_label, and no font is available to draw labels")
        self.cfg = cfg
        self.backend = backend
        self.generator = torch.Generator()
        self.generator.manual_seed(cfg.seed)
        self.index = {}

    def overlaps(self, extrinsics: torch.Tensor, intrinsics: torch.Tensor, shape) -> torch.Tensor:
        """overlap [v, v] f32 on the host: entry (i, j) is the share of camera i's rays that overlap image j, NaN outside the band.
        One view_overlap_counts call, one device-to-host copy."""
        v = extrinsics.shape[0]
        pairs = band_pairs(v, self.cfg.min_distance, self.cfg.max_distance)
        counts = view_overlap_counts(extrinsics, intrinsics, shape, pairs.to(extrinsics.device), backend=self.backend)
        table = torch.full((v, v), float("nan"), dtype=torch.float32)
        table[pairs[:, 0].long(), pairs[:, 1].long()] = overlap_from_counts(counts.cpu(), int(shape[0]) * int(shape[1]))
        return table

    def test_step(self, batch, batch_idx):
        b, v, _, h, w = batch["target"]["image"].shape
        assert b == 1
        extrinsics = batch["target"]["extrinsics"][0]
        intrinsics = batch["target"]["intrinsics"][0]
        scene = batch["scene"][0]
        table = self.overlaps(extrinsics, intrinsics, (h, w))

        context_indices = torch.randperm(v, generator=self.generator)
        for context_index in context_indices.tolist():
            # Step away from context view until the minimum overlap threshold is met.
            valid_indices = []
            for step in (1, -1):
                min_distance = self.cfg.min_distance
                max_distance = self.cfg.max_distance
                current_index = context_index + step * min_distance

                while 0 <= current_index < v:
                    # the rays of the current view on the context image, and the other way round
                    overlap_a = table[current_index, context_index]
                    overlap_b = table[context_index, current_index]

                    overlap = min(overlap_a, overlap_b)
                    delta = abs(current_index - context_index)

                    min_overlap = self.cfg.min_overlap
                    max_overlap = self.cfg.max_overlap
                    if min_overlap <= overlap <= max_overlap:
                        valid_indices.append((current_index, overlap_a, overlap_b))

                    # Stop once the camera has panned away too much.
                    if overlap < min_overlap or delta > max_distance:
                        break

                    current_index += step

            if valid_indices:
                # Pick a random valid view. Index the resulting views.
                num_options = len(valid_indices)
                chosen = torch.randint(0, num_options, size=tuple(), generator=self.generator)
                chosen, overlap_a, overlap_b = valid_indices[chosen]

                context_left = min(chosen, context_index)
                context_right = max(chosen, context_index)

                # Pick non-repeated random target views.
                while True:
                    target_views = torch.randint(context_left, context_right + 1, (self.cfg.num_target_views,), generator=self.generator)
                    if (target_views.unique(return_counts=True)[1] == 1).all():
                        break

                target = tuple(sorted(target_views.tolist()))
                self.index[scene] = IndexEntry(context=(context_left, context_right), target=target)
                break
        else:
            # This happens if no starting frame produces a valid evaluation example.
            self.index[scene] = None

    def save_index(self) -> None:
        self.cfg.output_path.mkdir(exist_ok=True, parents=True)
        with (self.cfg.output_path / "evaluation_index.json").open("w") as f:
            json.dump({k: None if v is None else asdict(v) for k, v in self.index.items()}, f, indent=4)
