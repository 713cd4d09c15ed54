"""The fifth compilation of csrc/env_kernels.hip (-DIRRL_EVAL_UNIT: the persistent policy-evaluation kernel in its two solver forms, object
env_kernels_l16ev) held to what tests/test_isa_pass_rt_unit.py holds the fourth to: hazard-free DPP instructions, and EnvParams / EnvState /
PolicyStepArgs / EvalArgs at the kernarg offsets IRRL_BIND_ARGS / IRRL_BIND_POLICY_ARGS / IRRL_BIND_EVAL_ARGS assume.  The unit's flags are part
of the library's source hash."""
import os

import pytest
import yaml

from high_speed_quadrupedal_locomotion_by_irrl_amd import build, isa_pass

EVAL_KERNELS = ("irrl_eval_persistent_kernel_l16", "irrl_eval_persistent_kernel_rt_l16")
LDS_BYTES = 160 * 1024     # a gfx950 workgroup's share


@pytest.fixture(scope="module")
def eval_assembly():
    build.build()
    path = os.path.join(build.CSRC, "_obj", "env_kernels_l16ev.s")
    if not os.path.exists(path):        # library reused from a previous build without its intermediates
        build.build(force=True)
    return open(path).read()


def _kernels(assembly):
    lines = assembly.split("\n")
    a = next(i for i, l in enumerate(lines) if l.strip() == ".amdgpu_metadata")
    b = next(i for i, l in enumerate(lines) if l.strip() == ".end_amdgpu_metadata")
    return yaml.safe_load("\n".join(lines[a + 1:b]))["amdhsa.kernels"]


def test_eval_unit_is_hazard_free(eval_assembly):
    lines = eval_assembly.splitlines(keepends=True)
    assert isa_pass.verify(lines) >= 400               # every DPP instruction, hand-placed and compiler-generated, of two kernels
    assert eval_assembly.count("v_fmac_f32_dpp") >= 40 # two env steps' worth of exchanges riding on the FMAs
    out, st = isa_pass.run(lines)
    assert st["wait_states_added"] == 0                # idempotent: nothing left to fix
    with pytest.raises(isa_pass.HazardError):
        isa_pass.verify([l for l in lines if not l.strip().startswith("s_nop")])


def test_eval_unit_holds_exactly_the_two_kernels_within_the_lds_and_register_budget(eval_assembly):
    kernels = _kernels(eval_assembly)
    assert sorted(k[".name"] for k in kernels) == sorted(EVAL_KERNELS)
    for k in kernels:
        print("%s: %d VGPR + AGPR (%d AGPR), %d B scratch, %d B LDS, %d spilled VGPR" % (
            k[".name"], k[".vgpr_count"], k[".agpr_count"], k[".private_segment_fixed_size"], k[".group_segment_fixed_size"], k[".vgpr_spill_count"]))
        assert k[".group_segment_fixed_size"] <= LDS_BYTES, k[".name"]
        assert k[".vgpr_count"] <= 512 and k[".vgpr_spill_count"] == 0, k[".name"]     # one wave per SIMD: its whole register file, nothing spilled
        assert k[".max_flat_workgroup_size"] == 256, k[".name"]


def test_eval_unit_kernarg_offsets_are_the_ones_the_kernels_assume(eval_assembly):
    for k in _kernels(eval_assembly):
        args = [x for x in k[".args"] if not x[".value_kind"].startswith("hidden_")]
        p, s = args[0], args[1]
        assert p[".value_kind"] == "by_value" and p[".offset"] == 0 and p[".size"] % 4 == 0 and p[".size"] >= 92 * 4, k[".name"]      # EnvParams first
        assert s[".value_kind"] == "by_value" and s[".size"] == 26 * 8 and s[".offset"] == (p[".size"] + 7) // 8 * 8, k[".name"]        # EnvState behind it
        assert [x[".value_kind"] for x in args[2:]] == ["global_buffer"] * 4 + ["by_value"] * 2, k[".name"]
        pa, ea = args[6], args[7]
        assert pa[".size"] > 200 and pa[".offset"] == (s[".offset"] + s[".size"] + 4 * 8 + 7) // 8 * 8, k[".name"]                       # PolicyStepArgs
        assert ea[".size"] > 200 and ea[".offset"] == (pa[".offset"] + pa[".size"] + 7) // 8 * 8, k[".name"]                            # EvalArgs behind it


def test_eval_unit_flags_enter_the_source_hash(monkeypatch):
    before = build.source_hash()
    monkeypatch.setattr(build, "EVAL_UNIT_FLAGS", build.EVAL_UNIT_FLAGS + ["-DIRRL_SOMETHING_ELSE"])
    assert build.source_hash() != before
