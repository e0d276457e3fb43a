"""ani_set_option (GPU, no compute call): every name the library accepts, one accepted value each, one refused value where a
name refuses any, and the refusal's text.  The rows are a literal copy of what the option code said before it became a table."""
import pytest

from lammps_ani_amd import ani_hip

# (name, an accepted value, a refused value or None, a fragment of the refusal)
OPTIONS = [
    ("prune_absent_species", 0, None, None),
    ("rdf_lanes", 64, 32, "ani_set_option: rdf_lanes is 16 or 64"),
    ("rdf_lds", 0, None, None),
    ("mlp_chain", 2, None, None),
    ("nbr_onepass", 0, None, None),
    ("out_force_accumulate", 1, None, None),
    ("nbr_sorted_rows", 0, None, None),
    ("nbr_half_cells", 1, None, None),
    ("reuse_build_list_upload", 1, None, None),
    ("mlp_fused", 3, 4, "mlp_fused must be 0, 1, 2 or 3"),
    ("aev_symmetric_radial", 0, None, None),
    ("aev_tickets_min", 0, -1, "aev_tickets_min must be >= 0"),
    ("aev_fused", 0, None, None),
    ("mlp_fused_gen", 0, 2, "mlp_fused_gen must be 0 or 1"),
    ("mlp_fused_rows", 64, 32, "mlp_fused_rows must be 0, 64 or 128"),
    ("mlp_fused_halves", 2, 3, "mlp_fused_halves must be 0, 1 or 2"),
    ("mlp_fused_schedule", 0, None, None),
    ("mlp_pipeline", 2, -1, "mlp_pipeline must be 0, 1 or 2"),
    ("mlp_arith", 2, 3, "mlp_arith must be 0 (fp32-input MFMA), 1 (bf16 x 3, exact) or 2 (fp16 x 2)"),
    ("mlp_split_bf16", 0, None, None),
    ("device_overwrite_forces", 1, None, None),
    ("profiling", 1, None, None),
    ("full_radial_capacity", 1, None, None),
]


@pytest.mark.gpu
def test_every_option_name_value_and_refusal(model_cache):
    ani = ani_hip.ANI(model_cache("tiny", 1, 7), 0, -1, True, True, True)
    try:
        assert len({name for name, *_ in OPTIONS}) == len(OPTIONS) == 23
        for name, good, bad, fragment in OPTIONS:
            ani.set_option(name, good)
            if bad is not None:
                with pytest.raises(ani_hip.AniError) as ei:
                    ani.set_option(name, bad)
                assert fragment in str(ei.value), (name, str(ei.value))
                ani.set_option(name, good)     # a refusal changes nothing: the name still takes its value
        for name in ("mlp_fuse", "mlp_fused ", "Profiling", ""):
            with pytest.raises(ani_hip.AniError) as ei:
                ani.set_option(name, 1)
            assert f"unknown option '{name}'" in str(ei.value)
    finally:
        ani.close()
