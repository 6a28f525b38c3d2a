"""Golden cases at 448 x 448 and 512 x 512 inputs (785 and 1025 tokens incl. CLS), in the form of the `*_micro_384` cases of
tests/_params.py: D = 128, depth 4, 2 heads, batch 2, weights and images from seeds.  Every family plus the dense DeiT at both sizes,
and keep_rate 0.9 at 512 x 512 for the clustering families (921 / 829 / 746 centres: beyond the 640 the kernels held before).
The fixtures (tests/golden/<name>.npz) come from tests/golden/gen_golden_hires.py, which runs the reference on these cases."""

_FAMILIES = {
    # family: (keep_rate, extra keys)
    "deit": ([1.0], dict(reduction_loc=[])),
    "topk": ([0.5], {}),
    "evit": ([0.7], {}),
    "tome": ([0.7], {}),
    "dyvit": ([0.7], {}),
    "sit": ([0.7], {}),
    "dpcknn": ([0.7], {}),
    "ats": ([0.8], {}),       # counts whose float grid has K - 1 points at both sizes (the K-point grids: test_hip_model.py)
    "sinkhorn": ([0.25], {}),
    "kmedoids": ([0.25], {}),
    "patchmerger": ([0.7], {}),
    "heuristic": ([0.7], dict(heuristic_pattern="l2", not_contiguous=True)),
}


def _case(family, img_size, seed, keep_rate, **extra):
    c = dict(family=family, embed_dim=128, depth=4, num_heads=2, num_classes=16, img_size=img_size, keep_rate=list(keep_rate),
             reduction_loc=[1, 2, 3], batch=2, wseed=seed, xseed=seed + 1, qkv_gain=6.0)
    c.update(extra)
    return c


HIRES_CASES = {}
for _i, (_fam, (_kr, _extra)) in enumerate(_FAMILIES.items()):
    for _j, _S in enumerate((448, 512)):
        HIRES_CASES[f"{_fam}_micro_{_S}"] = _case(_fam, _S, 3000 + 20 * _i + 2 * _j, _kr, **_extra)
# Heuristic's radius pattern (contiguous range, heuristic.py:157-181): the radius shrinks from the grid corner to min_radius
for _j, _S in enumerate((448, 512)):
    HIRES_CASES[f"heuristic_micro_{_S}_radius"] = _case("heuristic", _S, 3300 + 2 * _j, [0.7], heuristic_pattern="linf",
                                                        not_contiguous=False, min_radius=2.0)
# centre counts beyond 640 at 512 x 512 (1024 patch tokens x 0.9, 0.81, 0.729)
for _j, _fam in enumerate(("sinkhorn", "dpcknn", "kmedoids")):
    HIRES_CASES[f"{_fam}_micro_512_kr09"] = _case(_fam, 512, 3400 + 2 * _j, [0.9])
# seeds moved where the generator's tie-free assertions fired on the first choice
for _name, _seed in (("dyvit_micro_448", 4084), ("dyvit_micro_512", 4086), ("dpcknn_micro_512", 4152), ("dpcknn_micro_512_kr09", 4404),
                     ("ats_micro_448", 3152), ("kmedoids_micro_512_kr09", 3412)):
    HIRES_CASES[_name].update(wseed=_seed, xseed=_seed + 1)

# Not pinned by the CPU oracle test (test_hires_oracle.py); the executor tests (test_hires_parity.py) take them with their own near-tie rules.
# DPC-KNN and ATS: at 784 / 1024 tokens some centre or sample is decided by a gap at the rounding level of the matmul-form cdist, and
# which token wins there depends on the CPU's BLAS (the same fixture passed on one machine and failed on another).
ORACLE_NEAR_TIE = {n for n, c in HIRES_CASES.items() if c["family"] in ("dpcknn", "ats")}
# bf16x3 free-running: the centre gaps of DPC-KNN at 512 x 512 (down to 4e-6 relative) are below the ~1e-5 a split product carries;
# the fp32 executor holds this case exactly.
BF16X3_NEAR_TIE = {"dpcknn_micro_512"}
# test_hip_model.test_model_parity's ToMe and Heuristic legs are written for 197 tokens (they assert the 224 x 224 token counts);
# both families are held at these sizes by the fp32 and bf16x3 executor tests.
BF16_PARITY_224_ONLY = {n for n, c in HIRES_CASES.items() if c["family"] in ("tome", "heuristic")}
