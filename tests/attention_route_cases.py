"""The cases of tests/test_attention_routes_gpu.py: plain data, no torch.  tests/test_routes_cpu.py proves, without a GPU, that each case
reaches the route its id names (attention_route of vicasplat_amd/csrc/routes.h through tests/route_probe.cpp).

A case is (id, classes, make_case keywords).  Classes: f16, bf16, f32x (dtype 3), split (f32 in), sp (packed q | k | v in).  The first part of
an id is the route the case is meant to reach:
    res     attention_res_kernel            k1      attention_kernel<*,1>           k2      attention_kernel<*,2>
    split1  attention_split_kernel<1>       split2  attention_split_kernel<2>       sp      attention_sp_kernel<3>
    sweep / fam: every class; 16-bit: res when the case has no mask and no segments and fits the resident kernel, k1 otherwise;
    f32x: attention_f32_kernel; split: split1; sp: sp.
"""
ALL = ("f16", "bf16", "f32x", "split", "sp")

# The input families: name -> make_case keywords of tests/attention_f64.py (shape and storage are added per case).
FAMILIES = {
    "plain": dict(),
    "ragged": dict(mask="ragged"),
    "camera2": dict(mask="camera2"),
    "camera3": dict(mask="camera3"),
    "camera8": dict(mask="camera8"),
    "seg_prod2": dict(seg="prod2"),
    "seg_zero_first": dict(seg="zero_first"),
    "seg_uneven": dict(seg="uneven"),
    "seg_twice": dict(seg="twice"),
    "seg_overlap": dict(seg="overlap"),
    "seg_uneven_ragged": dict(seg="uneven", mask="ragged"),
    "seg_prod2_ragged": dict(seg="prod2", mask="ragged"),
    "plain_peaked": dict(regime="peaked"),
    "ragged_peaked": dict(mask="ragged", regime="peaked"),
    "seg_uneven_peaked": dict(seg="uneven", regime="peaked"),
    "seg_uneven_ragged_peaked": dict(seg="uneven", mask="ragged", regime="peaked"),
    "plain_uniform": dict(regime="uniform"),
    "ragged_uniform": dict(mask="ragged", regime="uniform"),
    "seg_uneven_ragged_uniform": dict(seg="uneven", mask="ragged", regime="uniform"),
    "plain_scale03": dict(scale=0.3),
    "ragged_scale03": dict(mask="ragged", scale=0.3),
    "seg_uneven_ragged_scale03": dict(seg="uneven", mask="ragged", scale=0.3),
}


def _cases():
    cs = []
    b16 = ("f16", "bf16")
    for Lq, Lk in [(1, 1), (257, 16), (384, 17), (257, 257), (384, 320), (1, 320)]:
        cs.append((f"res-Lq{Lq}-Lk{Lk}", b16, dict(nbatch=2, H=3, Lq=Lq, Lk=Lk)))
    cs.append(("k1-exit-Lk321", b16, dict(nbatch=2, H=3, Lq=257, Lk=321)))
    cs.append(("k1-exit-Lq385", b16, dict(nbatch=2, H=3, Lq=385, Lk=257)))
    cs.append(("k1-exit-257-ragged", b16, dict(nbatch=2, H=3, Lq=257, mask="ragged")))
    cs.append(("k1-exit-257-seg_prod2", b16, dict(nbatch=2, H=3, Lq=257, seg="prod2")))
    cs.append(("k2-1032-H16-nb4-plain", b16, dict(nbatch=4, H=16, Lq=1032)))            # 9 * 16 * 4 = 576 work-groups, last query tile 8 rows
    cs.append(("k2-1032-H16-nb4-camera8", b16, dict(nbatch=4, H=16, Lq=1032, mask="camera8")))
    cs.append(("split2-257-H16-nb11-plain", ("split",), dict(nbatch=11, H=16, Lq=257)))    # 3 * 16 * 11 = 528
    cs.append(("split2-257-H16-nb11-ragged", ("split",), dict(nbatch=11, H=16, Lq=257, mask="ragged")))
    cs.append(("split2-516-H16-nb7-plain", ("split",), dict(nbatch=7, H=16, Lq=516)))      # 5 * 16 * 7 = 560
    cs.append(("split1-257-H16-nb10-plain", ("split",), dict(nbatch=10, H=16, Lq=257)))    # 480: just below the count
    for Lq in (1, 95, 96, 97, 257, 1032):
        cs.append((f"sp-Lq{Lq}-plain", ("sp",), dict(nbatch=2, H=2, Lq=Lq)))
    for Lq in (97, 1032):
        cs.append((f"sp-Lq{Lq}-ragged", ("sp",), dict(nbatch=2, H=2, Lq=Lq, mask="ragged")))
    for L in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 258):
        for fam in ("plain", "ragged", "seg_uneven"):
            cs.append((f"sweep-L{L}-{fam}", ALL, dict(nbatch=2, H=2, Lq=L, **FAMILIES[fam])))
    for Lq, Lk in ((1, 300), (300, 1)):
        for fam in ("plain", "ragged"):
            cs.append((f"sweep-Lq{Lq}-Lk{Lk}-{fam}", ALL, dict(nbatch=2, H=2, Lq=Lq, Lk=Lk, **FAMILIES[fam])))
    for L in (100, 257):
        for fam, kw in FAMILIES.items():
            cs.append((f"fam-L{L}-{fam}", ALL, dict(nbatch=3, H=2, Lq=L, **kw)))
    return cs


CASES = _cases()

# test_permuting_batch_items_permutes_the_result: (id, class, make_case keywords)
PERMUTE_CASES = [
    ("sp-257-H4-nb8", "sp", dict(nbatch=8, H=4, Lq=257)),
    ("sp-96-H2-nb5-ragged", "sp", dict(nbatch=5, H=2, Lq=96, mask="ragged")),
    ("k2-1032-H16-nb4", "f16", dict(nbatch=4, H=16, Lq=1032)),
    ("split2-257-H16-nb11", "split", dict(nbatch=11, H=16, Lq=257, mask="ragged")),
]
