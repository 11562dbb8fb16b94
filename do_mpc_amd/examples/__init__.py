"""The four BASELINE workloads and four more of the reference's shipped NMPC examples (bicycle models, kite, rotating masses),
restated on do_mpc_amd's Model/MPC surface.

Each module has `build_model()` and `build_mpc(model, **settings_overrides)` plus `X0`, the
example's initial state.  Equations/settings follow the reference examples (cited per file);
the un-edited reference templates themselves run through do_mpc_amd.casadi_compat in
tests/test_reference_templates.py when /root/reference is present.
"""
from . import (batch_reactor, batch_reactor_lqr_dae, bicycle, cstr, cstr_ampc, cstr_lqr, dip, industrial_poly, kite, oscillating_masses, oscillating_masses_dae,  # noqa: F401
               oscillating_masses_lqr, rotating_masses, shape_family, triple_tank)

CASES = {"industrial_poly": industrial_poly, "CSTR": cstr, "batch_reactor": batch_reactor,
         "oscillating_masses": oscillating_masses, "kinematic_bicycle": bicycle.kinematic,
         "dynamic_bicycle": bicycle.dynamic, "kite": kite, "rotating_masses": rotating_masses,
         "oscillating_masses_dae": oscillating_masses_dae, "dip": dip, "triple_tank": triple_tank,
         "cstr_lqr": cstr_lqr, "oscillating_masses_lqr": oscillating_masses_lqr, "cstr_ampc": cstr_ampc,
         "batch_reactor_lqr_dae": batch_reactor_lqr_dae,
         # the synthetic shape family (no counterpart in the reference): the module with its default member, and every member by id
         "shape_family": shape_family}
CASES.update({"shape_family:" + mid: shape_family.member(mid) for mid in shape_family.MEMBERS})
BASELINE_CASES = ("industrial_poly", "CSTR", "batch_reactor", "oscillating_masses")
