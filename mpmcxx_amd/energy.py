"""ctypes binding of the C ABI (include/mpmc_energy.h) -- host-side mirror of the reference's energy surface.

`System` mirrors the part of the reference's `System` class that the energy hot path exposes
(reference src/System.h:314-402): ``energy()``, ``lj()``, ``coulombic()``, ``coulombic_real()``,
``coulombic_reciprocal()``, ``coulombic_self()``, ``polar()``, ``thole_field()``, ``thole_amatrix()`` and the
``observables`` it fills; errors surface as ``MpmcError(code)`` with the reference's integer error codes
(src/constants.h:108-147), the Python spelling of the reference's ``throw <int>``.

There is no CPU fallback: if the HIP library is missing or no device is present this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))

# status codes (include/mpmc_energy.h)
MPMC_OK = 0
ERR_UNSUPPORTED = 4004
ERR_INVALID_SETTING = 4000
DISP_DAMP, DISP_EXTRAPOLATE_C10, DISP_SCHMIDT = 1, 2, 4  # MPMC_DISP_* (mpmc_set_disp_expansion)
ERR_NO_DEVICE = -1
DAMPING = {"off": 0, "linear": 1, "exponential": 2, None: 2}
SOLVER = {"auto": 0, "matrix_free": 1, "compact": 2, "dense": 3}
K_NAMES = ["pair", "recip", "field", "tensor", "dipole_iter", "reduce", "dipole_far", "classes"]


class MpmcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mpmc error {code}: {msg}")
        self.code = code


class Options(C.Structure):
    _fields_ = [
        ("rd_only", C.c_int32), ("rd_lrc", C.c_int32), ("polarization", C.c_int32), ("polar_iterative", C.c_int32),
        ("polar_ewald", C.c_int32), ("polar_max_iter", C.c_int32), ("polar_gs", C.c_int32), ("polar_rrms", C.c_int32),
        ("damp_type", C.c_int32), ("ewald_kmax", C.c_int32), ("solver", C.c_int32), ("wolf", C.c_int32),
        ("polar_precision", C.c_double), ("polar_gamma", C.c_double), ("polar_damp", C.c_double),
        ("ewald_alpha", C.c_double), ("polar_ewald_alpha", C.c_double), ("unsupported_flags", C.c_uint64),
        ("feynman_hibbs", C.c_int32), ("feynman_hibbs_order", C.c_int32), ("temperature", C.c_double),
    ]


class Result(C.Structure):
    _fields_ = [
        ("energy", C.c_double), ("rd_energy", C.c_double), ("coulombic_energy", C.c_double), ("polarization_energy", C.c_double),
        ("vdw_energy", C.c_double), ("three_body_energy", C.c_double), ("kinetic_energy", C.c_double),
        ("es_real", C.c_double), ("es_recip", C.c_double), ("es_self", C.c_double),
        ("lj_pairs", C.c_double), ("lrc_pair", C.c_double), ("lrc_self", C.c_double),
        ("dipole_rrms", C.c_double), ("N", C.c_double), ("NU", C.c_double),
        ("n_pairs", C.c_int64), ("n_lj_in_cutoff", C.c_int64), ("n_es_in_cutoff", C.c_int64), ("n_intra", C.c_int64),
        ("n_rd_excluded", C.c_int64), ("n_es_excluded", C.c_int64), ("n_frozen", C.c_int64),
        ("polar_iterations", C.c_int32), ("iterator_failed", C.c_int32),
    ]

    def as_dict(self) -> Dict[str, float]:
        return {f: getattr(self, f) for f, _ in self._fields_}


class GibbsMove(C.Structure):
    _fields_ = [("movetype", C.c_int32 * 2), ("temperature", C.c_double), ("init_energy", C.c_double * 2), ("final_energy", C.c_double * 2),
                ("N", C.c_double * 2), ("volume", C.c_double * 2), ("checkpoint_volume_0", C.c_double)]


class DirectInfo(C.Structure):
    """mpmc_direct_info: the last direct dipole solve (`polar_iterative off`) of a context."""
    _fields_ = [("n_unknowns", C.c_int64), ("status", C.c_int64), ("residual", C.c_double), ("factor_bytes", C.c_int64)]


class RdModelInfo(C.Structure):
    """mpmc_rd_model_info: the last evaluation of a context with a non-default rd model."""
    _fields_ = [("form", C.c_int32), ("mixing", C.c_int32), ("n_terms", C.c_int64), ("n_tile_pairs", C.c_int64), ("n_tile_pairs_skipped", C.c_int64)]


class SilveraGoldmanInfo(C.Structure):
    """mpmc_silvera_goldman_info: the setting, and the last evaluation of a context with the Silvera-Goldman term."""
    _fields_ = [("enabled", C.c_int32), ("feynman_hibbs", C.c_int32), ("n_terms", C.c_int64), ("cutoff", C.c_double)]


# MPMC_RD_FORM_* / MPMC_RD_MIX_* and the reference keywords that select them
RD_FORM = {"lj": 0, "lj_buffered_14_7": 1, "dreiding": 2}
RD_MIX = {"lb": 0, "waldmanhagler": 1, "halgren_mixing": 2, "c6_mixing": 3}
RD_MODEL_KEYS = ("waldmanhagler", "halgren_mixing", "c6_mixing", "lj_buffered_14_7", "dreiding")


def rd_model_of(options: Dict[str, object]):
    """(form, mixing) of the reference keywords in `options`: dreiding wins over lj_buffered_14_7 (the dispatch order of System::energy,
    src/System.Energy.cpp:113-127), lj_buffered_14_7 does not switch Halgren mixing on (the reference only prints that it does), and more than
    one mixing rule is refused as the reference refuses it (SimulationControl.cpp:1706-1713)."""
    rules = [k for k in ("waldmanhagler", "halgren_mixing", "c6_mixing") if options.get(k)]
    if len(rules) > 1:
        raise MpmcError(ERR_INVALID_SETTING, "more than one mixing rule: " + " and ".join(rules))
    form = RD_FORM["dreiding"] if options.get("dreiding") else RD_FORM["lj_buffered_14_7"] if options.get("lj_buffered_14_7") else RD_FORM["lj"]
    return form, (RD_MIX[rules[0]] if rules else RD_MIX["lb"])


class AutorejectInfo(C.Structure):
    """mpmc_cavity_autoreject_info: the contact counts behind the last result delivered (evaluation, component call or trial)."""
    _fields_ = [("rules", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_double), ("repulsion", C.c_double), ("n_replaced", C.c_int64),
                ("n_absolute", C.c_int64), ("n_unmeasured_frozen", C.c_int64), ("absolute_penalty", C.c_double), ("returned_energy", C.c_double),
                ("tile_pairs_walked", C.c_int64), ("tile_pairs_skipped", C.c_int64)]


AUTOREJECT_SIGMA, AUTOREJECT_ABSOLUTE = 1, 2  # MPMC_AUTOREJECT_*
AUTOREJECT_KEYS = ("cavity_autoreject", "cavity_autoreject_absolute", "cavity_autoreject_scale", "cavity_autoreject_repulsion")


def autoreject_of(options: Dict[str, object]):
    """(rules, scale, repulsion) of the reference keywords in `options`; the reference's default scale is 0, which it refuses with a rule on
    (SimulationControl.cpp:2139-2154)."""
    on = lambda v: bool(v) and not (isinstance(v, str) and v.lower() in ("off", "0"))  # (1 / True / "on", as the readers and gen_box spell it)
    rules = (AUTOREJECT_SIGMA if on(options.get("cavity_autoreject")) else 0) | (AUTOREJECT_ABSOLUTE if on(options.get("cavity_autoreject_absolute")) else 0)
    return rules, float(options.get("cavity_autoreject_scale") or 0.0), float(options.get("cavity_autoreject_repulsion") or 0.0)


class RdCrystalInfo(C.Structure):
    """mpmc_rd_crystal_info: the last evaluation of a context with `rd_crystal` on."""
    _fields_ = [("order", C.c_int32), ("n_images", C.c_int32), ("cutoff", C.c_double), ("n_image_terms", C.c_int64), ("crystal_self", C.c_double)]


class EwaldFullInfo(C.Structure):
    """mpmc_ewald_full_info: the last evaluation of a context with `polar_ewald_full` on."""
    _fields_ = [("passes", C.c_int32), ("n_k", C.c_int32), ("n_real_pairs", C.c_int64), ("store_bytes", C.c_int64)]


PEF_VECTOR_KWEIGHT = 1  # MPMC_PEF_VECTOR_KWEIGHT


class RelaxInfo(C.Structure):
    """mpmc_relax_info: the last evaluation with a dipole solve of a context (mpmc_polar_relax_info)."""
    _fields_ = [("scheme", C.c_int32), ("zodid", C.c_int32), ("acted", C.c_int32), ("store_filled", C.c_int32), ("contractions", C.c_int64),
                ("last_weight", C.c_double)]


POLAR_RELAX = {"none": 0, "sor": 1, "esor": 2}  # MPMC_POLAR_RELAX_*
POLAR_RELAX_KEYS = ("polar_sor", "polar_esor", "polar_zodid")


def polar_relax_of(options: Dict[str, object]):
    """(scheme, zodid) of the option keys `polar_sor` / `polar_esor` / `polar_zodid`; both schemes together are refused as the reference
    refuses them (SimulationControl.cpp:2714-2730)"""
    sor, esor = bool(options.get("polar_sor")), bool(options.get("polar_esor"))
    if sor and esor:
        raise ValueError("polar_sor and polar_esor are both on")
    return POLAR_RELAX["sor"] if sor else POLAR_RELAX["esor"] if esor else POLAR_RELAX["none"], bool(options.get("polar_zodid"))


class GsRankedInfo(C.Structure):
    """mpmc_gs_ranked_info: the last evaluation with a dipole solve of a context (mpmc_polar_gs_ranked_info)."""
    _fields_ = [("enabled", C.c_int32), ("acted", C.c_int32), ("rmin", C.c_double), ("max_rank", C.c_int32), ("n_moved", C.c_int32),
                ("ranked_sweeps", C.c_int32), ("reserved", C.c_int32)]


class CavityResult(C.Structure):
    """mpmc_cavity_result: one update of the cavity-bias grid (mpmc_cavity_update)."""
    _fields_ = [("total_points", C.c_int64), ("cavities_open", C.c_int64), ("n_darts", C.c_int64), ("hits", C.c_int64),
                ("probability", C.c_double), ("cavity_volume", C.c_double)]


class UvtMove(C.Structure):
    """mpmc_uvt_move: what the ENSEMBLE_UVT branch of System::boltzmann_factor reads (mpmc_uvt_boltzmann_factor)."""
    _fields_ = [("movetype", C.c_int32), ("biased_move", C.c_int32), ("sorbate_count", C.c_int32), ("temperature", C.c_double), ("fugacity", C.c_double),
                ("volume", C.c_double), ("N", C.c_double), ("init_energy", C.c_double), ("final_energy", C.c_double), ("cavity_volume", C.c_double),
                ("avg_cavity_probability", C.c_double)]


MOVETYPE = {"insert": 0, "remove": 1, "displace": 2, "adiabatic": 3, "spinflip": 4, "volume": 5, "perturb_beads": 6}  # MPMC_MOVETYPE_*
CAVITY_KEYS = ("cavity_bias", "cavity_grid_size", "cavity_radius")
CAVITY_MAX_GRID = 128  # MPMC_CAVITY_MAX_GRID


class NptMove(C.Structure):
    """mpmc_npt_move: what the ENSEMBLE_NPT branch of System::boltzmann_factor reads (mpmc_npt_boltzmann_factor)."""
    _fields_ = [("movetype", C.c_int32), ("reserved", C.c_int32), ("temperature", C.c_double), ("pressure", C.c_double), ("N", C.c_double),
                ("init_energy", C.c_double), ("final_energy", C.c_double), ("volume_old", C.c_double), ("volume_new", C.c_double)]


class Timings(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("launches", C.c_int64 * 8)]


_lib = None


def lib():
    """load (building if needed) mpmcxx_amd/libmpmc_energy.so; raises if it cannot be produced."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MPMC_ENERGY_LIB") or _build.LIB  # override: same-box A/B of two builds (tools/ab_bench.sh)
    if not os.path.exists(path):
        if path != _build.LIB:
            raise FileNotFoundError(path)
        path = _build.build_library()
    L = C.CDLL(path)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    vp = C.c_void_p
    L.mpmc_abi_version.restype = C.c_int
    L.mpmc_device_count.argtypes = [C.POINTER(C.c_int)]
    if hasattr(L, "mpmc_device_synchronize") or not os.environ.get("MPMC_ENERGY_LIB"):  # (ABI 6)
        L.mpmc_device_synchronize.argtypes = [C.c_int]
        L.mpmc_device_name.argtypes = [C.c_int, C.c_char_p, C.c_int]
    L.mpmc_last_error.argtypes = [vp]
    L.mpmc_last_error.restype = C.c_char_p
    L.mpmc_pbc_compute.argtypes = [dp, dp, dp, dp]
    L.mpmc_default_options.argtypes = [C.POINTER(Options)]
    L.mpmc_default_options.restype = None
    L.mpmc_ctx_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.mpmc_ctx_destroy.argtypes = [vp]
    L.mpmc_set_box.argtypes = [vp, dp, dp, C.c_double, C.c_double]
    L.mpmc_set_options.argtypes = [vp, C.POINTER(Options)]
    L.mpmc_set_atoms.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, ip, ip, ip, dp]
    L.mpmc_update_positions.argtypes = [vp, C.c_int, C.c_int, dp]
    L.mpmc_set_positions_device.argtypes = [vp, vp]
    L.mpmc_energy.argtypes = [vp, C.POINTER(Result)]
    L.mpmc_energy_async.argtypes = [vp]
    L.mpmc_energy_wait.argtypes = [vp, C.POINTER(Result)]
    for name in ("mpmc_lj", "mpmc_coulombic", "mpmc_coulombic_real", "mpmc_coulombic_reciprocal", "mpmc_coulombic_self", "mpmc_polar"):
        getattr(L, name).argtypes = [vp, dp]
    if hasattr(L, "mpmc_set_axilrod_teller") or not os.environ.get("MPMC_ENERGY_LIB"):  # (an earlier build named by MPMC_ENERGY_LIB has no three-body term)
        L.mpmc_set_axilrod_teller.argtypes = [vp, C.c_int, C.c_int, dp, dp]
        L.mpmc_axilrod_teller.argtypes = [vp, dp]
    if hasattr(L, "mpmc_set_disp_expansion") or not os.environ.get("MPMC_ENERGY_LIB"):  # (likewise for the disp-expansion term)
        L.mpmc_set_disp_expansion.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp]
        L.mpmc_disp_expansion.argtypes = [vp, dp]
    L.mpmc_thole_field.argtypes = [vp, dp]
    L.mpmc_thole_amatrix.argtypes = [vp, C.c_int, C.c_int, dp]
    L.mpmc_get_dipoles.argtypes = [vp, dp, dp, dp]
    L.mpmc_update_com.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_int)]
    L.mpmc_pi_potential_local.argtypes = [C.POINTER(vp), C.c_int, dp, C.POINTER(Result), C.POINTER(C.c_int)]
    L.mpmc_pi_potential_local_host.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(dp), dp, C.POINTER(Result), C.POINTER(C.c_int)]
    L.mpmc_pi_finish.argtypes = [dp, C.c_int, dp]
    L.mpmc_last_batch_size.argtypes = [vp]
    L.mpmc_pi_chain_mass_length2.argtypes = [C.c_int, C.c_int, dp, dp, ip]
    L.mpmc_pi_chain_mass_length2.restype = C.c_double
    L.mpmc_pi_kinetic.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_double]
    L.mpmc_pi_kinetic.restype = C.c_double
    L.mpmc_pi_finish.restype = C.c_double
    L.mpmc_set_profiling.argtypes = [vp, C.c_int]
    L.mpmc_get_timings.argtypes = [vp, C.POINTER(Timings), C.c_int]
    L.mpmc_synchronize.argtypes = [vp]
    L.mpmc_memory_usage.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if hasattr(L, "mpmc_polar_direct_info") or not os.environ.get("MPMC_ENERGY_LIB"):
        L.mpmc_polar_direct_info.argtypes = [vp, C.POINTER(DirectInfo)]
    if hasattr(L, "mpmc_set_polar_wolf") or not os.environ.get("MPMC_ENERGY_LIB"):  # (likewise for the Wolf static field and the Palmo-Krimm correction)
        L.mpmc_set_polar_wolf.argtypes = [vp, C.c_int, C.c_double]
        L.mpmc_set_polar_palmo.argtypes = [vp, C.c_int]
        L.mpmc_polar_palmo_info.argtypes = [vp, dp, dp]
    if hasattr(L, "mpmc_set_rd_crystal") or not os.environ.get("MPMC_ENERGY_LIB"):  # (likewise for the lattice-summed Lennard-Jones)
        L.mpmc_set_rd_crystal.argtypes = [vp, C.c_int, C.c_int]
        L.mpmc_rd_crystal_info.argtypes = [vp, C.POINTER(RdCrystalInfo)]
    if hasattr(L, "mpmc_set_rd_model") or not os.environ.get("MPMC_ENERGY_LIB"):  # (likewise for the rd model)
        L.mpmc_set_rd_model.argtypes = [vp, C.c_int, C.c_int]
        L.mpmc_rd_model_info.argtypes = [vp, C.POINTER(RdModelInfo)]
    if hasattr(L, "mpmc_set_silvera_goldman") or not os.environ.get("MPMC_ENERGY_LIB"):  # (likewise for the Silvera-Goldman potential)
        L.mpmc_set_silvera_goldman.argtypes = [vp, C.c_int]
        L.mpmc_silvera_goldman_info.argtypes = [vp, C.POINTER(SilveraGoldmanInfo)]
    if hasattr(L, "mpmc_set_cavity_autoreject") or not os.environ.get("MPMC_ENERGY_LIB"):  # (likewise for cavity_autoreject)
        L.mpmc_set_cavity_autoreject.argtypes = [vp, C.c_int, C.c_double, C.c_double]
        L.mpmc_cavity_autoreject_info.argtypes = [vp, C.POINTER(AutorejectInfo)]
        if hasattr(L, "mpmc_insert_candidates_contacts") or not os.environ.get("MPMC_ENERGY_LIB"):
            L.mpmc_insert_candidates_contacts.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if hasattr(L, "mpmc_set_polar_ewald_full") or not os.environ.get("MPMC_ENERGY_LIB"):  # (likewise for the fully periodic dipole solve)
        L.mpmc_set_polar_ewald_full.argtypes = [vp, C.c_int, C.c_int]
        L.mpmc_polar_ewald_full_info.argtypes = [vp, C.POINTER(EwaldFullInfo)]
    if hasattr(L, "mpmc_set_polar_relax") or not os.environ.get("MPMC_ENERGY_LIB"):  # (likewise for the relaxed updates and zeroth-order dipoles)
        L.mpmc_set_polar_relax.argtypes = [vp, C.c_int, C.c_int]
        L.mpmc_polar_relax_info.argtypes = [vp, C.POINTER(RelaxInfo)]
    if hasattr(L, "mpmc_set_polar_gs_ranked") or not os.environ.get("MPMC_ENERGY_LIB"):  # (likewise for the ranked Gauss-Seidel sweeps)
        L.mpmc_set_polar_gs_ranked.argtypes = [vp, C.c_int]
        L.mpmc_polar_gs_ranked_info.argtypes = [vp, C.POINTER(GsRankedInfo)]
        L.mpmc_polar_gs_ranked_get.argtypes = [vp, ip, ip]
        L.mpmc_debug_gs_rank_order.argtypes = [vp, ip, ip]
        if hasattr(L, "mpmc_debug_gs_ranked_pair_stats") or not os.environ.get("MPMC_ENERGY_LIB"):
            L.mpmc_debug_gs_ranked_pair_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    L.mpmc_get_tile_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    L.mpmc_trial_begin.argtypes = [vp, C.c_int, C.c_int, dp]
    L.mpmc_trial_energy.argtypes = [vp, C.POINTER(Result)]
    L.mpmc_trial_accept.argtypes = [vp]
    L.mpmc_trial_reject.argtypes = [vp]
    if hasattr(L, "mpmc_trial_insert_begin") or not os.environ.get("MPMC_ENERGY_LIB"):  # (an earlier build named by MPMC_ENERGY_LIB has no exchange trials)
        L.mpmc_trial_insert_begin.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, ip, ip, dp]
        L.mpmc_trial_remove_begin.argtypes = [vp, C.c_int, C.c_int]
    if hasattr(L, "mpmc_insert_candidates") or not os.environ.get("MPMC_ENERGY_LIB"):  # (an earlier build named by MPMC_ENERGY_LIB has no candidate batches)
        L.mpmc_insert_candidates.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, ip, ip, dp, C.POINTER(Result)]
        L.mpmc_debug_insert_batch_counts.argtypes = [vp, C.POINTER(C.c_longlong)]
    if hasattr(L, "mpmc_set_cavity_grid") or not os.environ.get("MPMC_ENERGY_LIB"):  # (an earlier build named by MPMC_ENERGY_LIB has no cavity grid)
        L.mpmc_set_cavity_grid.argtypes = [vp, C.c_int, C.c_double]
        L.mpmc_cavity_update.argtypes = [vp, C.c_int, dp, C.POINTER(CavityResult)]
        L.mpmc_cavity_point.argtypes = [vp, C.c_int64, dp]
        L.mpmc_cavity_get.argtypes = [vp, ip, dp, ip]
        L.mpmc_cavity_num_darts.argtypes = [C.c_double]
        L.mpmc_cavity_grid_point.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
        L.mpmc_cavity_r2_threshold.argtypes = [C.c_double]
        L.mpmc_cavity_r2_threshold.restype = C.c_double
        L.mpmc_uvt_boltzmann_factor.argtypes = [C.POINTER(UvtMove), dp]
        L.mpmc_debug_cavity_times.argtypes = [vp, dp]
    if hasattr(L, "mpmc_trial_volume_begin") or not os.environ.get("MPMC_ENERGY_LIB"):  # (an earlier build named by MPMC_ENERGY_LIB has no volume trials)
        L.mpmc_trial_volume_begin.argtypes = [vp, C.c_double]
        L.mpmc_trial_volume_get.argtypes = [vp, dp, dp, dp, dp, dp]
        L.mpmc_debug_volume_trial_counts.argtypes = [vp, C.POINTER(C.c_longlong)]
        L.mpmc_npt_boltzmann_factor.argtypes = [C.POINTER(NptMove), dp]
        L.mpmc_debug_device_positions.argtypes = [vp, dp]
    L.mpmc_gibbs_energy.argtypes = [vp, vp, C.POINTER(Result), C.POINTER(Result)]
    L.mpmc_gibbs_boltzmann_factor.argtypes = [C.POINTER(GibbsMove), dp, dp]
    L.mpmc_rccl_version.argtypes = [C.POINTER(C.c_int)]
    if hasattr(L, "mpmc_rccl_library_path") or not os.environ.get("MPMC_ENERGY_LIB"):  # (ABI 6)
        L.mpmc_rccl_library_path.argtypes = []
        L.mpmc_rccl_library_path.restype = C.c_char_p
    L.mpmc_comm_unique_id.argtypes = [C.c_char_p]
    L.mpmc_comm_init_rank.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.mpmc_comm_init_all.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int)]
    L.mpmc_comm_destroy.argtypes = [vp]
    L.mpmc_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpmc_comm_last_error.argtypes = [vp]
    L.mpmc_comm_last_error.restype = C.c_char_p
    L.mpmc_comm_allgather_f64.argtypes = [vp, dp, C.c_int64, dp]
    L.mpmc_pi_gather_beads.argtypes = [vp, dp, C.c_int, C.c_int, dp]
    if hasattr(L, "mpmc_hint_in_flight") or not os.environ.get("MPMC_ENERGY_LIB"):
        L.mpmc_hint_in_flight.argtypes = [vp, C.c_int]
    if hasattr(L, "mpmc_set_dipoles_on_demand") or not os.environ.get("MPMC_ENERGY_LIB"):  # (an older build under the A/B override lacks it)
        L.mpmc_set_dipoles_on_demand.argtypes = [vp, C.c_int]
    L.mpmc_pi_allreduce.argtypes = [C.POINTER(vp), C.c_int, dp, C.POINTER(Result), C.POINTER(C.c_int)]
    if hasattr(L, "mpmc_pi_allreduce_info") or not os.environ.get("MPMC_ENERGY_LIB"):  # (an older build under the A/B override lacks the ABI-5 entry)
        L.mpmc_pi_allreduce_info.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mpmc_debug_configure.argtypes = [vp, C.c_char_p, C.c_double]
    L.mpmc_debug_last_pair_kernel.argtypes = [vp]
    L.mpmc_debug_last_trial_was_full.argtypes = [vp]
    L.mpmc_debug_erfc_table.argtypes = [C.c_double, dp, dp]
    if hasattr(L, "mpmc_debug_erfc_table_field") or not os.environ.get("MPMC_ENERGY_LIB"):
        L.mpmc_debug_erfc_table_field.argtypes = [C.c_double, dp]
    L.mpmc_debug_pair_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    L.mpmc_debug_time_panel.argtypes = [vp, C.c_int, dp]
    L.mpmc_debug_time_pair.argtypes = [vp, C.c_int, dp]
    _lib = L
    return L


def configure(key: str, value: float):
    """measurement / A-B switch for contexts created AFTER this call (mpmc_debug_configure with a null context)."""
    rc = lib().mpmc_debug_configure(None, key.encode(), float(value))
    if rc != MPMC_OK:
        raise MpmcError(rc, f"mpmc_debug_configure: unknown key or bad value: {key}={value}")


def _dp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def device_count() -> int:
    n = C.c_int(0)
    lib().mpmc_device_count(C.byref(n))
    return n.value


def device_synchronize(device: int = 0):
    """everything this process enqueued on `device` has finished (mpmc_device_synchronize)."""
    rc = lib().mpmc_device_synchronize(int(device))
    if rc != MPMC_OK:
        raise MpmcError(rc, f"mpmc_device_synchronize({device})")


def device_name(device: int = 0) -> str:
    buf = C.create_string_buffer(256)
    rc = lib().mpmc_device_name(int(device), buf, 256)
    if rc != MPMC_OK:
        raise MpmcError(rc, f"mpmc_device_name({device})")
    return buf.value.decode()


def pbc_compute(basis: np.ndarray):
    """PeriodicBoundary::update: returns (reciprocal(3,3), volume, cutoff)."""
    b = np.ascontiguousarray(basis, dtype=np.float64).reshape(9)
    R = np.zeros(9)
    vol, cut = C.c_double(), C.c_double()
    rc = lib().mpmc_pbc_compute(_dp(b), _dp(R), C.byref(vol), C.byref(cut))
    if rc != MPMC_OK:
        raise MpmcError(rc, "invalid box")
    return R.reshape(3, 3), vol.value, cut.value


def make_options(opts: Dict[str, object]) -> Options:
    o = Options()
    lib().mpmc_default_options(C.byref(o))
    for k in ("rd_only", "rd_lrc", "polarization", "polar_iterative", "polar_ewald", "polar_max_iter", "polar_gs", "polar_rrms", "ewald_kmax",
              "wolf", "feynman_hibbs", "feynman_hibbs_order"):
        if k in opts and opts[k] is not None:
            setattr(o, k, int(opts[k]))
    for k in ("polar_precision", "polar_gamma", "polar_damp", "temperature"):
        if k in opts and opts[k] is not None:
            setattr(o, k, float(opts[k]))
    for k in ("ewald_alpha", "polar_ewald_alpha"):
        v = opts.get(k)
        setattr(o, k, float(v) if v is not None else 0.0)
    dt = opts.get("damp_type")
    o.damp_type = DAMPING[dt] if not isinstance(dt, int) else dt
    sv = opts.get("solver", "auto")
    o.solver = SOLVER[sv] if not isinstance(sv, int) else sv
    o.unsupported_flags = int(opts.get("unsupported_flags", 0))
    return o


class System:
    """Device-resident state of one box (one reference `System` / one PI bead)."""

    def __init__(self, atoms: Dict[str, np.ndarray], basis: np.ndarray, options: Dict[str, object], device: int = 0,
                 max_atoms: Optional[int] = None):
        L = lib()
        self._L = L
        self._h = C.c_void_p()
        n = int(np.asarray(atoms["pos"]).shape[0])
        rc = L.mpmc_ctx_create(int(device), int(max_atoms or n), C.byref(self._h))
        if rc != MPMC_OK:
            raise MpmcError(rc, (L.mpmc_last_error(None) or b"").decode())
        self.n = n
        self._obs: Dict[str, float] = {}
        self._obs_lazy = None  # (ctypes Result array, index): turned into a dict when somebody looks (the PI loops fill 32 of these per step)
        self.set_box(basis)
        self.set_options(options)
        self.set_atoms(atoms)

    # -- plumbing -------------------------------------------------------------------------------------------
    @property
    def observables(self) -> Dict[str, float]:
        if self._obs_lazy is not None:
            arr, i = self._obs_lazy
            self._obs, self._obs_lazy = arr[i].as_dict(), None
        return self._obs

    @observables.setter
    def observables(self, d):
        self._obs, self._obs_lazy = d, None

    def _check(self, rc: int):
        if rc != MPMC_OK:
            raise MpmcError(rc, (self._L.mpmc_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.mpmc_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def configure(self, key: str, value: float):
        """measurement / A-B switch of THIS context (see mpmc_debug_configure in csrc/context.cpp)."""
        self._check(self._L.mpmc_debug_configure(self._h, key.encode(), float(value)))

    def last_trial_was_full(self) -> bool:
        """whether the last trial move ran a full evaluation of the trial configuration (True) or per-move delta energies (False)."""
        return self._L.mpmc_debug_last_trial_was_full(self._h) == 1

    def last_pair_kernel(self) -> str:
        return "sweep" if self._L.mpmc_debug_last_pair_kernel(self._h) == 1 else "fused"

    # -- state ------------------------------------------------------------------------------------------------
    def _volume_closed(self):
        """the four state calls close an open volume trial in the library (also where they then refuse their arguments): the object's flag
        takes the library's own answer"""
        if getattr(self, "_volume", False):
            self._volume = self._L.mpmc_trial_volume_get(self._h, None, None, None, None, None) == MPMC_OK

    def set_box(self, basis: np.ndarray):
        b = np.ascontiguousarray(basis, dtype=np.float64).reshape(9)
        try:
            self._check(self._L.mpmc_set_box(self._h, _dp(b), None, 0.0, 0.0))
        finally:
            self._volume_closed()
        self.basis = b.reshape(3, 3).copy()

    def set_options(self, options: Dict[str, object]):
        self._opts = make_options(options)
        try:
            self._check(self._L.mpmc_set_options(self._h, C.byref(self._opts)))
        finally:
            self._volume_closed()
        self.options = dict(options)
        # `polar_wolf` / `polar_palmo` are switches of their own in the library and follow the options here (only when some options named them:
        # a library of before this term, named by MPMC_ENERGY_LIB, is never asked)
        if "polar_wolf" in options or "polar_palmo" in options or getattr(self, "_polar_wolf_set", False):
            self._polar_wolf_set = True
            alpha = options.get("polar_wolf_alpha")
            self.set_polar_wolf(bool(options.get("polar_wolf")), 0.0 if alpha is None else float(alpha))
            self.set_polar_palmo(bool(options.get("polar_palmo")))
        # `rd_crystal` likewise (reference default of rd_crystal_order: 0, which it refuses with the term on)
        if "rd_crystal" in options or getattr(self, "_rd_crystal_set", False):
            self._rd_crystal_set = True
            self.set_rd_crystal(bool(options.get("rd_crystal")), int(options.get("rd_crystal_order") or 0))
        # the rd model likewise: `waldmanhagler` / `halgren_mixing` / `c6_mixing` and `lj_buffered_14_7` / `dreiding`
        if any(k in options for k in RD_MODEL_KEYS) or getattr(self, "_rd_model_set", False):
            self._rd_model_set = True
            self.set_rd_model(*rd_model_of(options))
        # `sg` likewise: the Silvera-Goldman potential
        if "sg" in options or getattr(self, "_sg_set", False):
            self._sg_set = True
            self.set_silvera_goldman(bool(options.get("sg")))
        # cavity_autoreject likewise: `cavity_autoreject`, `cavity_autoreject_absolute`, `cavity_autoreject_scale`, `cavity_autoreject_repulsion`
        if any(k in options for k in AUTOREJECT_KEYS) or getattr(self, "_autoreject_set", False):
            self._autoreject_set = True
            self.set_cavity_autoreject(*autoreject_of(options))

        # `polar_ewald_full` likewise ("polar_ewald_full_flags": PEF_VECTOR_KWEIGHT or 0; the reference has no keyword for it)
        if "polar_ewald_full" in options or getattr(self, "_polar_ewald_full_set", False):
            self._polar_ewald_full_set = True
            self.set_polar_ewald_full(bool(options.get("polar_ewald_full")), int(options.get("polar_ewald_full_flags") or 0))
        # `polar_sor` / `polar_esor` / `polar_zodid` likewise (gamma stays the option polar_gamma)
        if any(k in options for k in POLAR_RELAX_KEYS) or getattr(self, "_polar_relax_set", False):
            self._polar_relax_set = True
            self.set_polar_relax(*polar_relax_of(options))
        # `polar_gs_ranked` likewise
        if "polar_gs_ranked" in options or getattr(self, "_polar_gs_ranked_set", False):
            self._polar_gs_ranked_set = True
            self.set_polar_gs_ranked(bool(options.get("polar_gs_ranked")))

        # `cavity_bias` likewise: the grid is switched on or off only when the options name one of its keys
        if any(k in options for k in CAVITY_KEYS) or getattr(self, "_cavity_set", False):
            self._cavity_set = True
            on = bool(options.get("cavity_bias"))
            self.set_cavity_grid(int(options.get("cavity_grid_size") or 0) if on else 0, float(options.get("cavity_radius") or 0.0))

    def set_atoms(self, atoms: Dict[str, np.ndarray]):
        f = lambda k: np.ascontiguousarray(atoms[k], dtype=np.float64)
        g = lambda k: np.ascontiguousarray(atoms[k], dtype=np.int32)
        pos = f("pos").reshape(-1)
        n = pos.size // 3
        disp = g("has_disp") if "has_disp" in atoms else None
        mass = f("mass") if "mass" in atoms else None
        try:
            self._check(self._L.mpmc_set_atoms(self._h, n, _dp(pos), _dp(f("charge")), _dp(f("polarizability")), _dp(f("epsilon")),
                                               _dp(f("sigma")), _ip(g("mol_id")), _ip(g("frozen")), _ip(disp), _dp(mass)))
        finally:
            self._volume_closed()
        self.n = n
        # the object's own copy of the list: accepted trials and update_positions keep it current (set_positions_device does not: the positions
        # stay on the device)
        self._atoms = {k: np.array(v) for k, v in atoms.items()}
        self._atoms["pos"] = np.array(pos.reshape(n, 3))
        self._exchange = self._move = None
        # the library discards three-body coefficients with every atom list: the term follows the options (`axilrod_teller on`)
        if self.options.get("axilrod_teller"):
            mk = bool(self.options.get("midzuno_kihara_approx"))
            key = "c6" if mk else "c9"
            if key not in atoms:
                raise ValueError(f"axilrod_teller is on but the atoms carry no {key!r} column")
            self.set_axilrod_teller(True, atoms[key] if mk else None, None if mk else atoms[key], midzuno_kihara_approx=mk)
        # likewise the disp-expansion coefficients (`disp_expansion on`)
        if self.options.get("disp_expansion"):
            for key in ("c6", "c8", "c10"):
                if key not in atoms:
                    raise ValueError(f"disp_expansion is on but the atoms carry no {key!r} column")
            o = self.options
            self.set_disp_expansion(True, atoms["c6"], atoms["c8"], atoms["c10"], damp=bool(o.get("damp_dispersion")),
                                    extrapolate_c10=bool(o.get("extrapolate_disp_coeffs")), schmidt=bool(o.get("schmidt_ff")))

    def set_disp_expansion(self, enabled: bool, c6: Optional[np.ndarray] = None, c8: Optional[np.ndarray] = None, c10: Optional[np.ndarray] = None,
                           damp: bool = False, extrapolate_c10: bool = False, schmidt: bool = False):
        """switch the disp-expansion repulsion/dispersion term on (per-atom c6, c8, c10 in atomic units; the atoms' epsilon / sigma are its
        alpha / r0) or off (mpmc_set_disp_expansion).  It replaces the LJ part of rd_energy."""
        a = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (c6, c8, c10)]
        flags = (DISP_DAMP if damp else 0) | (DISP_EXTRAPOLATE_C10 if extrapolate_c10 else 0) | (DISP_SCHMIDT if schmidt else 0)
        self._check(self._L.mpmc_set_disp_expansion(self._h, int(bool(enabled)), flags, _dp(a[0]), _dp(a[1]), _dp(a[2])))

    def set_rd_crystal(self, enabled: bool, order: int = 0):
        """`rd_crystal`: Lennard-Jones summed over the (2 order - 1)^3 periodic images of the cell with the cutoff 2 * cutoff * (order - 0.5)
        (mpmc_set_rd_crystal).  It replaces the LJ sum of rd_energy."""
        self._check(self._L.mpmc_set_rd_crystal(self._h, int(bool(enabled)), int(order)))

    def rd_crystal_info(self) -> Dict[str, object]:
        """order, n_images, cutoff, n_image_terms and crystal_self of the last evaluation with the term on (mpmc_rd_crystal_info)"""
        v = RdCrystalInfo()
        self._check(self._L.mpmc_rd_crystal_info(self._h, C.byref(v)))
        return {k: getattr(v, k) for k, _ in RdCrystalInfo._fields_}

    # -- the cavity-bias grid of uVT moves (System::cavity_update_grid, reference src/System.Cavity.cpp) ---------------
    def set_cavity_grid(self, grid_size: int, radius: float = 0.0):
        """`cavity_bias`: a grid_size^3 grid of sphere centres of the given radius (mpmc_set_cavity_grid); grid_size = 0 switches it off"""
        self._check(self._L.mpmc_set_cavity_grid(self._h, int(grid_size), float(radius)))
        self._cavity_grid = int(grid_size)

    def cavity_update(self, dart_frac: Optional[np.ndarray] = None) -> Dict[str, float]:
        """one cavity_update_grid over the accepted atom list (mpmc_cavity_update).  dart_frac: (n_darts, 3) of the caller's `-0.5 + get_rand()`
        draws in draw order (None or empty: no darts, the volume is NaN as in the reference).  Returns total_points, cavities_open, n_darts,
        hits, probability and cavity_volume."""
        d = None if dart_frac is None else np.ascontiguousarray(dart_frac, dtype=np.float64).reshape(-1, 3)
        n_darts = 0 if d is None else int(d.shape[0])
        r = CavityResult()
        self._check(self._L.mpmc_cavity_update(self._h, n_darts, _dp(d) if n_darts else None, C.byref(r)))
        return {k: getattr(r, k) for k, _ in CavityResult._fields_}

    def cavity_point(self, rank: int) -> np.ndarray:
        """the rank-th empty sphere centre of the last update in the reference's enumeration order (mpmc_cavity_point)"""
        pos = np.zeros(3)
        self._check(self._L.mpmc_cavity_point(self._h, int(rank), _dp(pos)))
        return pos

    def cavity_grid(self):
        """(occupancy (G, G, G) int32, centres (G, G, G, 3), flat indices of the empty centres ascending) of the last update (mpmc_cavity_get)"""
        G = int(getattr(self, "_cavity_grid", 0))
        occ = np.zeros(G ** 3, dtype=np.int32)
        pos = np.zeros((G ** 3, 3))
        open_index = np.zeros(G ** 3, dtype=np.int32)
        self._check(self._L.mpmc_cavity_get(self._h, _ip(occ), _dp(pos), None))
        n_open = int(np.count_nonzero(occ == 0))
        self._check(self._L.mpmc_cavity_get(self._h, None, None, _ip(open_index)))
        return occ.reshape(G, G, G), pos.reshape(G, G, G, 3), open_index[:n_open].copy()

    def cavity_times(self) -> Dict[str, float]:
        """device milliseconds of the last cavity_update made under set_profiling(True) (mpmc_debug_cavity_times)"""
        ms = np.zeros(3)
        self._check(self._L.mpmc_debug_cavity_times(self._h, _dp(ms)))
        return {"occupancy": float(ms[0]), "compact": float(ms[1]), "darts": float(ms[2])}

    def set_rd_model(self, form=0, mixing=0):
        """The rd model (mpmc_set_rd_model): a potential form (RD_FORM: "lj", "lj_buffered_14_7", "dreiding", or its number) and a mixing rule
        (RD_MIX: "lb", "waldmanhagler", "halgren_mixing", "c6_mixing").  ("lj", "lb") restores the plain term."""
        f = RD_FORM[form] if isinstance(form, str) else int(form)
        m = RD_MIX[mixing] if isinstance(mixing, str) else int(mixing)
        self._check(self._L.mpmc_set_rd_model(self._h, f, m))

    def rd_model_info(self) -> Dict[str, object]:
        """form, mixing, n_terms, n_tile_pairs and n_tile_pairs_skipped of the last evaluation with a non-default model (mpmc_rd_model_info)"""
        v = RdModelInfo()
        self._check(self._L.mpmc_rd_model_info(self._h, C.byref(v)))
        return {k: getattr(v, k) for k, _ in RdModelInfo._fields_}

    def set_silvera_goldman(self, enabled: bool = True):
        """The Silvera-Goldman H2 potential (mpmc_set_silvera_goldman): sg() in place of lj(), no electrostatics, no polarization."""
        self._check(self._L.mpmc_set_silvera_goldman(self._h, 1 if enabled else 0))

    def silvera_goldman_info(self) -> Dict[str, object]:
        """enabled, and feynman_hibbs, n_terms and cutoff of the last evaluation with the term (mpmc_silvera_goldman_info)"""
        v = SilveraGoldmanInfo()
        self._check(self._L.mpmc_silvera_goldman_info(self._h, C.byref(v)))
        return {k: getattr(v, k) for k, _ in SilveraGoldmanInfo._fields_}

    def set_cavity_autoreject(self, rules: int = 0, scale: float = 0.0, repulsion: float = 0.0):
        """cavity_autoreject (mpmc_set_cavity_autoreject): rules = AUTOREJECT_SIGMA | AUTOREJECT_ABSOLUTE (0: off), scale in (0, 1]."""
        self._check(self._L.mpmc_set_cavity_autoreject(self._h, int(rules), float(scale), float(repulsion)))
        self._autoreject_on = int(rules) != 0

    def cavity_autoreject_info(self) -> Dict[str, object]:
        """rules, scale, repulsion, n_replaced, n_absolute, n_unmeasured_frozen, absolute_penalty, returned_energy, tile_pairs_walked and
        tile_pairs_skipped behind the last result delivered (mpmc_cavity_autoreject_info)"""
        v = AutorejectInfo()
        self._check(self._L.mpmc_cavity_autoreject_info(self._h, C.byref(v)))
        return {k: getattr(v, k) for k, _ in AutorejectInfo._fields_ if k != "reserved"}

    def insert_candidates_contacts(self, n_cand: int):
        """(n_replaced[n_cand], n_absolute[n_cand]) of the last insert_candidates batch: the contact counts of each candidate's trial
        composition, as cavity_autoreject_info gives them behind the single insertion trial (mpmc_insert_candidates_contacts)"""
        r, a = np.zeros(int(n_cand), dtype=np.int64), np.zeros(int(n_cand), dtype=np.int64)
        self._check(self._L.mpmc_insert_candidates_contacts(self._h, int(n_cand), r.ctypes.data_as(C.POINTER(C.c_int64)), a.ctypes.data_as(C.POINTER(C.c_int64))))
        return r, a

    def _returned(self, energy: float) -> float:
        """what System::energy() returns: the observables' energy, plus the absolute-rule penalty of cavity_autoreject when a rule is on"""
        if not getattr(self, "_autoreject_on", False):
            return energy
        return self.cavity_autoreject_info()["returned_energy"]

    def set_polar_relax(self, scheme=0, zodid: bool = False):
        """`polar_sor` / `polar_esor` (scheme "sor" / "esor" or POLAR_RELAX[...]; "none" / 0 switches off) and `polar_zodid`
        (mpmc_set_polar_relax); gamma is the option polar_gamma."""
        self._check(self._L.mpmc_set_polar_relax(self._h, POLAR_RELAX[scheme] if isinstance(scheme, str) else int(scheme), int(bool(zodid))))

    def polar_relax_info(self) -> Dict[str, float]:
        """scheme, zodid, acted, store_filled, contractions and last_weight of the last evaluation with a dipole solve (mpmc_polar_relax_info)"""
        v = RelaxInfo()
        self._check(self._L.mpmc_polar_relax_info(self._h, C.byref(v)))
        return {k: getattr(v, k) for k, _ in RelaxInfo._fields_}

    def set_polar_gs_ranked(self, enabled: bool):
        """`polar_gs_ranked`: Gauss-Seidel sweeps that run in descending rank order from the second iteration on (mpmc_set_polar_gs_ranked)"""
        self._check(self._L.mpmc_set_polar_gs_ranked(self._h, int(bool(enabled))))

    def polar_gs_ranked_info(self) -> Dict[str, float]:
        """enabled, acted, rmin, max_rank, n_moved and ranked_sweeps of the last evaluation with a dipole solve (mpmc_polar_gs_ranked_info)"""
        v = GsRankedInfo()
        self._check(self._L.mpmc_polar_gs_ranked_info(self._h, C.byref(v)))
        return {k: getattr(v, k) for k, _ in GsRankedInfo._fields_ if k != "reserved"}

    def polar_gs_ranked(self):
        """(rank_metric[n], order[n]) of the last evaluation under the setting, int32, in the caller's atom order; order[p] is the atom swept
        p-th from the second iteration on (mpmc_polar_gs_ranked_get)"""
        rank, order = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        self._check(self._L.mpmc_polar_gs_ranked_get(self._h, _ip(rank), _ip(order)))
        return rank, order

    def set_polar_ewald_full(self, enabled: bool, flags: int = 0):
        """`polar_ewald_full`: the induced field of the dipole solve as an Ewald sum as well (mpmc_set_polar_ewald_full); it replaces the
        whole solve.  flags: PEF_VECTOR_KWEIGHT for the intended reciprocal-space weight instead of the reference's scalar one."""
        self._check(self._L.mpmc_set_polar_ewald_full(self._h, int(bool(enabled)), int(flags)))

    def ewald_full_info(self) -> Dict[str, int]:
        """passes, n_k, n_real_pairs and store_bytes of the last evaluation with the term on (mpmc_polar_ewald_full_info)"""
        v = EwaldFullInfo()
        self._check(self._L.mpmc_polar_ewald_full_info(self._h, C.byref(v)))
        return {k: getattr(v, k) for k, _ in EwaldFullInfo._fields_}

    def set_polar_wolf(self, enabled: bool, polar_wolf_alpha: float = 0.0):
        """`polar_wolf`: the static field of the dipole solve as a Wolf sum with damping parameter polar_wolf_alpha in [0, 1]
        (mpmc_set_polar_wolf); it applies whenever polar_ewald is off."""
        self._check(self._L.mpmc_set_polar_wolf(self._h, int(bool(enabled)), float(polar_wolf_alpha)))

    def set_dipoles_on_demand(self, enabled: bool):
        """energy() / energy_async() of a fixed-count Jacobi solve stop at the iterations the energy needs; dipoles() runs the rest
        (mpmc_set_dipoles_on_demand; the pi_* loops always work this way)"""
        self._check(self._L.mpmc_set_dipoles_on_demand(self._h, int(bool(enabled))))

    def set_polar_palmo(self, enabled: bool):
        """`polar_palmo`: the Palmo-Krimm correction to the polarization energy (mpmc_set_polar_palmo)"""
        self._check(self._L.mpmc_set_polar_palmo(self._h, int(bool(enabled))))

    def palmo_info(self):
        """(correction, ef_induced_change[n][3]) of the last evaluation with a dipole solve (mpmc_polar_palmo_info); the correction is
        already part of polarization_energy, and exactly 0 under Jacobi iterations and under the direct solve."""
        v = C.c_double(0.0)
        d = np.zeros((self.n, 3))
        self._check(self._L.mpmc_polar_palmo_info(self._h, C.byref(v), _dp(d)))
        return v.value, d

    def set_axilrod_teller(self, enabled: bool, c6: Optional[np.ndarray] = None, c9: Optional[np.ndarray] = None,
                           midzuno_kihara_approx: bool = False):
        """switch the Axilrod-Teller three-body term on (per-atom c9, or c6 under the Midzuno-Kihara form) or off (mpmc_set_axilrod_teller)"""
        a6 = None if c6 is None else np.ascontiguousarray(c6, dtype=np.float64)
        a9 = None if c9 is None else np.ascontiguousarray(c9, dtype=np.float64)
        self._check(self._L.mpmc_set_axilrod_teller(self._h, int(bool(enabled)), int(bool(midzuno_kihara_approx)), _dp(a6), _dp(a9)))

    def update_positions(self, first: int, pos: np.ndarray):
        p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1)
        try:
            self._check(self._L.mpmc_update_positions(self._h, int(first), p.size // 3, _dp(p)))
        finally:
            self._volume_closed()
        if getattr(self, "_atoms", None) is not None:
            self._atoms["pos"][int(first):int(first) + p.size // 3] = p.reshape(-1, 3)

    def set_positions_device(self, data_ptr: int):
        """positions from device memory ([n][3] fp64).  The caller synchronizes the stream that produced them first (torch: `torch.cuda.current_stream().synchronize()`);
        the library reads them on its own stream and is done with the buffer when this returns."""
        self._check(self._L.mpmc_set_positions_device(self._h, C.c_void_p(data_ptr)))

    # -- double System::energy() (reference src/System.Energy.cpp:19) ---------------------------------------------
    def energy(self) -> float:
        r = Result()
        self._check(self._L.mpmc_energy(self._h, C.byref(r)))
        self.observables = r.as_dict()
        return self._returned(r.energy)

    def hint_in_flight(self, n: int):
        """scheduling hint for energy_async: how many evaluations the caller keeps in flight together with this one (mpmc_hint_in_flight)."""
        self._check(self._L.mpmc_hint_in_flight(self._h, int(n)))

    def energy_async(self):
        self._check(self._L.mpmc_energy_async(self._h))

    def energy_wait(self) -> float:
        r = Result()
        self._check(self._L.mpmc_energy_wait(self._h, C.byref(r)))
        self.observables = r.as_dict()
        return self._returned(r.energy)

    # -- trial moves (reference: per-pair recalculate_energy cache, src/System.cpp:1211-1224) ------------------------------
    def trial_energy(self, first: int, pos: np.ndarray) -> float:
        """energy of the configuration in which atoms first.. take the positions `pos`; follow with accept() or reject()."""
        p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1)
        self._check(self._L.mpmc_trial_begin(self._h, int(first), p.size // 3, _dp(p)))
        self._exchange, self._move = None, (int(first), p.reshape(-1, 3))
        r = Result()
        rc = self._L.mpmc_trial_energy(self._h, C.byref(r))
        if rc != MPMC_OK:
            self._L.mpmc_trial_reject(self._h)
            self._check(rc)
        self.trial_observables = r.as_dict()
        return self._returned(r.energy)

    @property
    def atoms(self) -> Dict[str, np.ndarray]:
        """the object's own copy of the atom list: what set_atoms was given, followed by update_positions and every accepted trial"""
        return self._atoms

    def _trial(self):
        r = Result()
        rc = self._L.mpmc_trial_energy(self._h, C.byref(r))
        if rc != MPMC_OK:
            msg = (self._L.mpmc_last_error(self._h) or b"").decode()
            self._L.mpmc_trial_reject(self._h)
            self._exchange = None
            raise MpmcError(rc, msg)
        self.trial_observables = r.as_dict()
        return self._returned(r.energy)

    def trial_insert_energy(self, at_index: int, mol_atoms: Dict[str, np.ndarray]) -> float:
        """energy of the composition with ONE more molecule: the atoms of `mol_atoms` (the keys of the atoms dict; mol_id is not read, the
        molecule gets an id of its own) in front of atom at_index (a molecule boundary, or n: appended); follow with accept() or reject()."""
        f = lambda k: np.ascontiguousarray(mol_atoms[k], dtype=np.float64)
        g = lambda k: np.ascontiguousarray(mol_atoms[k], dtype=np.int32)
        own = self._atoms
        pos = f("pos").reshape(-1)
        m = pos.size // 3
        disp = g("has_disp") if "has_disp" in mol_atoms else None
        mass = f("mass") if "mass" in mol_atoms else None
        self._check(self._L.mpmc_trial_insert_begin(self._h, int(at_index), m, _dp(pos), _dp(f("charge")), _dp(f("polarizability")), _dp(f("epsilon")),
                                                    _dp(f("sigma")), _ip(g("frozen")), _ip(disp), _dp(mass)))
        mol = {k: np.asarray(mol_atoms[k]) if k in mol_atoms else np.zeros((m,) + own[k].shape[1:], dtype=own[k].dtype) for k in own}
        mol["pos"] = pos.reshape(m, 3)
        mol["mol_id"] = np.full(m, int(np.max(own["mol_id"])) + 1, dtype=own["mol_id"].dtype)
        self._exchange, self._move = (int(at_index), 0, mol), None
        return self._trial()

    def insert_candidates(self, mol_atoms: Dict[str, np.ndarray], positions: np.ndarray) -> List[Dict[str, float]]:
        """the observables of `n_cand` trial insertions of ONE molecule, evaluated in one launch chain behind one wait: `mol_atoms` as for
        trial_insert_energy (its "pos" is not read), `positions` an (n_cand, m, 3) array of poses.  Entry c is what trial_insert_energy at pose
        c followed by reject() leaves in trial_observables, bit for bit.  Opens no trial and changes nothing of the accepted configuration."""
        f = lambda k: np.ascontiguousarray(mol_atoms[k], dtype=np.float64)
        g = lambda k: np.ascontiguousarray(mol_atoms[k], dtype=np.int32)
        m = int(np.asarray(mol_atoms["charge"]).size)
        pos = np.ascontiguousarray(positions, dtype=np.float64)
        if pos.ndim != 3 or pos.shape[1:] != (m, 3):
            raise ValueError(f"insert_candidates: positions must be (n_cand, {m}, 3), got {pos.shape}")
        n_cand = int(pos.shape[0])
        disp = g("has_disp") if "has_disp" in mol_atoms else None
        mass = f("mass") if "mass" in mol_atoms else None
        out = (Result * max(n_cand, 1))()
        self._check(self._L.mpmc_insert_candidates(self._h, m, n_cand, _dp(pos.reshape(-1)), _dp(f("charge")), _dp(f("polarizability")), _dp(f("epsilon")),
                                                   _dp(f("sigma")), _ip(g("frozen")), _ip(disp), _dp(mass), out))
        return [out[c].as_dict() for c in range(n_cand)]

    def insert_batch_counts(self):
        """(calls of insert_candidates that ran, candidates they evaluated) since the context was created (mpmc_debug_insert_batch_counts)"""
        v = (C.c_longlong * 2)()
        if self._L.mpmc_debug_insert_batch_counts(self._h, v) != 0:
            raise MpmcError(-1, "mpmc_debug_insert_batch_counts: no context")
        return int(v[0]), int(v[1])

    def trial_remove_energy(self, first: int, count: int) -> float:
        """energy of the composition without the molecule that occupies atoms [first, first + count); follow with accept() or reject()."""
        self._check(self._L.mpmc_trial_remove_begin(self._h, int(first), int(count)))
        self._exchange, self._move = (int(first), int(count), None), None
        return self._trial()

    def trial_volume_energy(self, scale: float) -> float:
        """energy of the configuration with every basis element times `scale` and every molecule shifted rigidly by com * scale - com
        (System::volume_change); follow with accept() or reject().  The atoms need masses."""
        self._check(self._L.mpmc_trial_volume_begin(self._h, float(scale)))
        self._exchange, self._move, self._volume = None, None, True
        try:
            return self._trial()
        except MpmcError:
            self._volume = False
            raise

    def trial_volume_state(self) -> Dict[str, object]:
        """the open volume trial's cell and positions (mpmc_trial_volume_get): basis (3, 3), reciprocal (3, 3), volume, cutoff, pos (n, 3)"""
        b, r, pos = np.zeros(9), np.zeros(9), np.zeros((self.n, 3))
        vol, cut = C.c_double(), C.c_double()
        self._check(self._L.mpmc_trial_volume_get(self._h, _dp(b), _dp(r), C.byref(vol), C.byref(cut), _dp(pos)))
        return {"basis": b.reshape(3, 3), "reciprocal": r.reshape(3, 3), "volume": vol.value, "cutoff": cut.value, "pos": pos}

    def device_positions(self) -> np.ndarray:
        """(diagnostics) the positions resident on the device, original atom order: the trial's while an evaluated volume trial is open"""
        pos = np.zeros((self.n, 3))
        self._check(self._L.mpmc_debug_device_positions(self._h, _dp(pos)))
        return pos

    def volume_trial_counts(self) -> Dict[str, int]:
        """volume trials evaluated, accepted and rejected, and evaluations made from inside a reject (mpmc_debug_volume_trial_counts)"""
        v = (C.c_longlong * 4)()
        if self._L.mpmc_debug_volume_trial_counts(self._h, v) != 0:
            raise MpmcError(-1, "mpmc_debug_volume_trial_counts: no context")
        return {"evaluated": int(v[0]), "accepted": int(v[1]), "rejected": int(v[2]), "reject_evaluations": int(v[3])}

    def accept(self):
        vol_state = self.trial_volume_state() if getattr(self, "_volume", False) else None  # (valid until the accept)
        self._check(self._L.mpmc_trial_accept(self._h))
        self.observables = dict(self.trial_observables)
        if vol_state is not None:  # the object's own cell and positions follow an accepted volume trial
            self.basis = vol_state["basis"].copy()
            if getattr(self, "_atoms", None) is not None:
                self._atoms["pos"][:] = vol_state["pos"]
            self._volume = False
        if getattr(self, "_exchange", None) is not None:  # the object's own atom arrays follow an accepted exchange
            at, n_remove, mol = self._exchange
            own = self.atoms
            for k in own:
                kept = np.delete(own[k], np.s_[at:at + n_remove], axis=0)
                own[k] = kept if mol is None else np.insert(kept, at, mol[k], axis=0)
            self.n = int(own["pos"].shape[0])
            self._exchange = None
        elif getattr(self, "_move", None) is not None:
            first, p = self._move
            self._atoms["pos"][first:first + p.shape[0]] = p
        self._move = None

    def reject(self):
        try:
            self._check(self._L.mpmc_trial_reject(self._h))
        finally:  # (whatever the library answers, "no trial move is open" included, the object holds no trial afterwards)
            self._exchange = self._move = None
            self._volume = False

    def _scalar(self, fn) -> float:
        v = C.c_double()
        self._check(fn(self._h, C.byref(v)))
        return v.value

    def lj(self) -> float:
        return self._scalar(self._L.mpmc_lj)

    def axilrod_teller(self) -> float:
        return self._scalar(self._L.mpmc_axilrod_teller)

    def disp_expansion(self) -> float:
        return self._scalar(self._L.mpmc_disp_expansion)

    def coulombic(self) -> float:
        return self._scalar(self._L.mpmc_coulombic)

    def coulombic_real(self) -> float:
        return self._scalar(self._L.mpmc_coulombic_real)

    def coulombic_reciprocal(self) -> float:
        return self._scalar(self._L.mpmc_coulombic_reciprocal)

    def coulombic_self(self) -> float:
        return self._scalar(self._L.mpmc_coulombic_self)

    def polar(self) -> float:
        return self._scalar(self._L.mpmc_polar)

    def thole_field(self) -> np.ndarray:
        E = np.zeros((self.n, 3))
        self._check(self._L.mpmc_thole_field(self._h, _dp(E)))
        return E

    def thole_amatrix(self, row0: int = 0, nrows: Optional[int] = None) -> np.ndarray:
        nrows = 3 * self.n - row0 if nrows is None else nrows
        A = np.zeros((nrows, 3 * self.n))
        self._check(self._L.mpmc_thole_amatrix(self._h, int(row0), int(nrows), _dp(A)))
        return A

    def dipoles(self):
        mu, E, F = np.zeros((self.n, 3)), np.zeros((self.n, 3)), np.zeros((self.n, 3))
        self._check(self._L.mpmc_get_dipoles(self._h, _dp(mu), _dp(E), _dp(F)))
        return mu, E, F

    def update_com(self):
        nm = C.c_int(0)
        com = np.zeros((self.n, 3))
        wcom = np.zeros((self.n, 3))
        wpos = np.zeros((self.n, 3))
        self._check(self._L.mpmc_update_com(self._h, _dp(com), _dp(wcom), _dp(wpos), C.byref(nm)))
        return com[: nm.value], wcom[: nm.value], wpos

    # -- measurement --------------------------------------------------------------------------------------------
    def set_profiling(self, on: bool):
        self._check(self._L.mpmc_set_profiling(self._h, 1 if on else 0))

    def timings(self, reset: bool = False) -> Dict[str, Dict[str, float]]:
        t = Timings()
        self._check(self._L.mpmc_get_timings(self._h, C.byref(t), 1 if reset else 0))
        return {K_NAMES[i]: {"ms": t.ms[i], "launches": int(t.launches[i])} for i in range(len(K_NAMES))}

    def synchronize(self):
        self._check(self._L.mpmc_synchronize(self._h))

    def tile_stats(self) -> Dict[str, int]:
        """tile-pair classes of the last evaluation (see mpmc_get_tile_stats)."""
        a = (C.c_int64 * 4)()
        self._check(self._L.mpmc_get_tile_stats(self._h, a))
        return {"tile_pairs": a[0], "thole_stored": a[1], "thole_far": a[2], "beyond_cutoff": a[3]}

    def pair_stats(self) -> Dict[str, int]:
        """exact atom-pair counts behind the tile-pair classes of the last evaluation (mpmc_debug_pair_stats)."""
        a = (C.c_int64 * 12)()
        self._check(self._L.mpmc_debug_pair_stats(self._h, a))
        keys = ["pairs", "pairs_stored", "pairs_far", "pairs_beyond_cutoff", "nonuniform_dims_x_pairs_stored", "nonuniform_dims_x_pairs_far",
                "pairs_swept", "nonuniform_dims_x_pairs_swept", "tile_pairs", "tile_pairs_stored", "tile_pairs_far", "tile_pairs_beyond_cutoff"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def gs_ranked_pair_stats(self) -> Dict[str, int]:
        """tile-pair classes of the ranked view the last evaluation under `polar_gs_ranked` swept (mpmc_debug_gs_ranked_pair_stats)."""
        a = (C.c_int64 * 6)()
        self._check(self._L.mpmc_debug_gs_ranked_pair_stats(self._h, a))
        keys = ["tile_pairs", "tile_pairs_off_diagonal", "tile_pairs_far", "tile_pairs_beyond_cutoff", "tile_pairs_common_image", "tile_pairs_shifted"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def time_kernel(self, which: str, reps: int = 100) -> float:
        """ms per launch of the dominant kernels of the LAST evaluation, `reps` launches back to back between one pair of HIP events on the
        context's stream: which = "panel" (Jacobi contraction) | "pair" (pair sweep)."""
        v = C.c_double(0.0)
        fn = self._L.mpmc_debug_time_panel if which == "panel" else self._L.mpmc_debug_time_pair
        self._check(fn(self._h, int(reps), C.byref(v)))
        return v.value

    def last_batch_size(self) -> int:
        """systems that shared each launch of the dipole iterations in the last evaluation (pi_potential_local batches compatible beads)."""
        return int(self._L.mpmc_last_batch_size(self._h))

    def memory_usage(self):
        a, b = C.c_int64(), C.c_int64()
        self._check(self._L.mpmc_memory_usage(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def direct_info(self) -> Dict[str, float]:
        """the last direct dipole solve (`polar_iterative off`): unknowns, status (0, or the 1-based index of the first non-positive
        pivot), relative residual max|E0 - A mu| / max|E0|, bytes held by the factor."""
        d = DirectInfo()
        self._check(self._L.mpmc_polar_direct_info(self._h, C.byref(d)))
        return {f: getattr(d, f) for f, _ in d._fields_}


class ResultList:
    """per-bead results of a PI loop: the ctypes array the library filled, turned into dicts on access (a 30-field dict per bead and step
    is 1 % of a 32-bead step when nobody reads it)."""

    def __init__(self, arr, n: int):
        self._arr, self._n = arr, n

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._arr[k].as_dict() for k in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        return self._arr[i].as_dict()

    def __iter__(self):
        return (self._arr[k].as_dict() for k in range(self._n))

    def table4(self) -> np.ndarray:
        """(n, 4) = {rd, coulombic, polarization, vdw} per bead -- what PI_calculate_potential combines (PathIntegral.cpp:763-766)."""
        raw = np.frombuffer(self._arr, dtype=np.float64, count=self._n * (C.sizeof(Result) // 8)).reshape(self._n, C.sizeof(Result) // 8)
        return np.ascontiguousarray(raw[:, 1:5])  # fields 1..4 of mpmc_result: rd_energy, coulombic_energy, polarization_energy, vdw_energy


def _adopt(beads, res, n):
    per = ResultList(res, n)
    for i, b in enumerate(beads):
        b._obs_lazy = (res, i)
    return per


def pi_potential_local(beads: Sequence[System], host_positions: Optional[Sequence[np.ndarray]] = None):
    """local leg of SimulationControl::PI_calculate_potential (reference PathIntegral.cpp:752-805):
    returns (sums4 = ordered sums of {rd, coulombic, polarization, vdw} over this rank's beads, per-bead results, failed).
    host_positions: one C-contiguous (n, 3) float64 array per bead -- the coordinates travel inside the call
    (mpmc_pi_potential_local_host: bead b's upload overlaps the evaluation of the beads in front of it)."""
    L = lib()
    n = len(beads)
    arr = (C.c_void_p * max(n, 1))(*[b.handle for b in beads])
    sums = np.zeros(4)
    res = (Result * max(n, 1))()
    failed = C.c_int(0)
    if host_positions is not None:
        if len(host_positions) != n:
            raise ValueError("host_positions: one array per bead")
        keep = [np.ascontiguousarray(p, dtype=np.float64) for p in host_positions]
        ptrs = (C.POINTER(C.c_double) * max(n, 1))(*[_dp(p) for p in keep])
        rc = L.mpmc_pi_potential_local_host(arr, n, ptrs, _dp(sums), res, C.byref(failed))
    else:
        rc = L.mpmc_pi_potential_local(arr, n, _dp(sums), res, C.byref(failed))
    if rc != MPMC_OK:
        msg = b""
        for b in beads:
            msg = L.mpmc_last_error(b.handle) or msg
        raise MpmcError(rc, msg.decode())
    return sums, _adopt(beads, res, n), bool(failed.value)


def gibbs_energy(box_a: System, box_b: System):
    """both boxes of a Gibbs ensemble (reference SimulationControl.Gibbs.cpp:179-180): enqueued together, waited for together; the boxes
    usually live on two devices (System(..., device=0) / System(..., device=1)).  Returns (E_a, E_b)."""
    ra, rb = Result(), Result()
    rc = lib().mpmc_gibbs_energy(box_a.handle, box_b.handle, C.byref(ra), C.byref(rb))
    if rc != MPMC_OK:
        raise MpmcError(rc, ((lib().mpmc_last_error(box_a.handle) or b"") + b" / " + (lib().mpmc_last_error(box_b.handle) or b"")).decode())
    box_a.observables, box_b.observables = ra.as_dict(), rb.as_dict()
    return ra.energy, rb.energy


def gibbs_boltzmann_factor(movetype, temperature, init_energy, final_energy, N, volume, checkpoint_volume_0, current=(float("nan"), float("nan"))):
    """SimulationControl::boltzmann_factor_NVT_Gibbs (reference Gibbs.cpp:358-522).  Returns (status, [bf_a, bf_b], [energy_a, energy_b]);
    entries the reference leaves untouched come back as `current` / the final energies."""
    m = GibbsMove()
    m.movetype[0], m.movetype[1] = int(movetype[0]), int(movetype[1])
    m.temperature = float(temperature)
    for k in range(2):
        m.init_energy[k], m.final_energy[k], m.N[k], m.volume[k] = float(init_energy[k]), float(final_energy[k]), float(N[k]), float(volume[k])
    m.checkpoint_volume_0 = float(checkpoint_volume_0)
    bf = np.array(current, dtype=np.float64)
    en = np.array(final_energy, dtype=np.float64)
    rc = lib().mpmc_gibbs_boltzmann_factor(C.byref(m), _dp(bf), _dp(en))
    return rc, bf, en


# ---- the host-only entry points of the cavity grid and the uVT acceptance factor (no device needed) ------------------------------------
def cavity_num_darts(volume: float) -> int:
    """darts update_cavity_volume throws at a cell of this volume: (int)(volume * 0.1) (mpmc_cavity_num_darts)"""
    return int(lib().mpmc_cavity_num_darts(float(volume)))


def cavity_grid_point(basis: np.ndarray, grid_size: int, i: int, j: int, k: int) -> np.ndarray:
    """sphere centre (i, j, k) of a grid_size^3 grid in the cell `basis`, the reference's arithmetic (mpmc_cavity_grid_point)"""
    b = np.ascontiguousarray(basis, dtype=np.float64).reshape(9)
    pos = np.zeros(3)
    rc = lib().mpmc_cavity_grid_point(_dp(b), int(grid_size), int(i), int(j), int(k), _dp(pos))
    if rc != MPMC_OK:
        raise MpmcError(rc, f"mpmc_cavity_grid_point: ({i}, {j}, {k}) outside a grid of {grid_size}")
    return pos


def cavity_r2_threshold(radius: float) -> float:
    """the smallest double whose correctly rounded square root is >= radius (mpmc_cavity_r2_threshold)"""
    return float(lib().mpmc_cavity_r2_threshold(float(radius)))


def uvt_boltzmann_factor(movetype, temperature, fugacity, volume, N, init_energy, final_energy, sorbate_count=1, biased_move=False, cavity_volume=0.0,
                         avg_cavity_probability=0.0):
    """the ENSEMBLE_UVT branch of System::boltzmann_factor (reference src/System.MonteCarlo.cpp:1358-1422).  movetype: a MOVETYPE name or
    number.  Returns (status, boltzmann_factor)."""
    m = UvtMove()
    m.movetype = MOVETYPE[movetype] if isinstance(movetype, str) else int(movetype)
    m.biased_move, m.sorbate_count = int(bool(biased_move)), int(sorbate_count)
    m.temperature, m.fugacity, m.volume, m.N = float(temperature), float(fugacity), float(volume), float(N)
    m.init_energy, m.final_energy = float(init_energy), float(final_energy)
    m.cavity_volume, m.avg_cavity_probability = float(cavity_volume), float(avg_cavity_probability)
    bf = C.c_double(float("nan"))
    rc = lib().mpmc_uvt_boltzmann_factor(C.byref(m), C.byref(bf))
    return rc, bf.value


def npt_boltzmann_factor(movetype, temperature, pressure, N, init_energy, final_energy, volume_old, volume_new) -> float:
    """the ENSEMBLE_NPT branch of System::boltzmann_factor (mpmc_npt_boltzmann_factor).  movetype: a MOVETYPE name or number; "volume" and "displace" have a factor"""
    movetype = MOVETYPE[movetype] if isinstance(movetype, str) else int(movetype)
    m = NptMove(movetype, 0, float(temperature), float(pressure), float(N), float(init_energy), float(final_energy), float(volume_old),
                float(volume_new))
    bf = C.c_double()
    rc = lib().mpmc_npt_boltzmann_factor(C.byref(m), C.byref(bf))
    if rc != MPMC_OK:
        raise MpmcError(rc, f"mpmc_npt_boltzmann_factor: move type {int(movetype)} has no NPT acceptance factor")
    return bf.value


def pi_allreduce(beads: Sequence[System]):
    """SimulationControl::PI_calculate_potential for ONE process that drives several GPUs (bead b usually on device b mod G): evaluation with
    one host thread per device, per-bead values gathered over RCCL (ncclCommInitAll communicator), ordered sum s = 0..P-1.
    Returns (sums4, per-bead results, failed) like pi_potential_local."""
    L = lib()
    n = len(beads)
    arr = (C.c_void_p * max(n, 1))(*[b.handle for b in beads])
    sums = np.zeros(4)
    res = (Result * max(n, 1))()
    failed = C.c_int(0)
    rc = L.mpmc_pi_allreduce(arr, n, _dp(sums), res, C.byref(failed))
    if rc != MPMC_OK:
        raise MpmcError(rc, ((L.mpmc_last_error(beads[0].handle) if beads else b"") or L.mpmc_comm_last_error(None) or b"").decode())
    return sums, _adopt(beads, res, n), bool(failed.value)


def pi_allreduce_info(beads: Sequence[System]):
    """(number of distinct devices the beads live on, size of the process-wide RCCL communicator pi_allreduce made for them; 0 = not yet)."""
    n = len(beads)
    arr = (C.c_void_p * max(n, 1))(*[b.handle for b in beads])
    nd, nr = C.c_int(0), C.c_int(0)
    rc = lib().mpmc_pi_allreduce_info(arr, n, C.byref(nd), C.byref(nr))
    if rc != MPMC_OK:
        raise MpmcError(rc, "mpmc_pi_allreduce_info")
    return nd.value, nr.value


def rccl_version() -> int:
    v = C.c_int(0)
    rc = lib().mpmc_rccl_version(C.byref(v))
    if rc != MPMC_OK:
        raise MpmcError(rc, (lib().mpmc_comm_last_error(None) or b"").decode())
    return v.value


def rccl_library_path() -> str:
    """the file RCCL's entry points were resolved from and why that copy (mpmc_rccl_library_path); "" if RCCL could not be opened."""
    return (lib().mpmc_rccl_library_path() or b"").decode()


def loaded_rocm_libs() -> Dict[str, list]:
    """the ROCm runtime libraries mapped into THIS process (/proc/self/maps): {"libamdhip64": [paths], "librccl": [...], ...}.
    One path per name = one ROCm in the process (what a rank of the multi-GPU job must show)."""
    names = ("libamdhip64", "librccl", "libhsa-runtime64", "librocm_smi64", "libmpmc_energy", "libtorch_hip")
    found: Dict[str, list] = {k: [] for k in names}
    try:
        with open("/proc/self/maps") as f:
            for ln in f:
                path = ln.split(None, 5)[-1].strip() if ln.count("/") else ""
                base = os.path.basename(path)
                for k in names:
                    if base.startswith(k + ".so") and path not in found[k]:
                        found[k].append(path)
    except OSError:
        pass
    return {k: v for k, v in found.items() if v}


class Comm:
    """RCCL communicator of the C ABI, one process per GPU: rank 0 makes the id (`Comm.unique_id()`), the launcher's own channel carries
    the 128 bytes to the other ranks (bench.py: torch.distributed's store), every rank constructs `Comm(n_ranks, rank, id, device)`."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(Comm.ID_BYTES)
        rc = lib().mpmc_comm_unique_id(buf)
        if rc != MPMC_OK:
            raise MpmcError(rc, (lib().mpmc_comm_last_error(None) or b"").decode())
        return buf.raw

    def __init__(self, n_ranks: int, rank: int, uid: bytes, device: int):
        self._L = lib()
        self._h = C.c_void_p()
        if len(uid) != Comm.ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        rc = self._L.mpmc_comm_init_rank(C.byref(self._h), int(n_ranks), int(rank), uid, int(device))
        if rc != MPMC_OK:
            raise MpmcError(rc, (self._L.mpmc_comm_last_error(None) or b"").decode())
        self.n_ranks, self.rank, self.device = int(n_ranks), int(rank), int(device)

    def _check(self, rc: int):
        if rc != MPMC_OK:
            raise MpmcError(rc, (self._L.mpmc_comm_last_error(self._h) or b"").decode())

    def allgather(self, local: np.ndarray) -> np.ndarray:
        """(count,) fp64 of this rank -> (n_ranks, count) in rank order."""
        a = np.ascontiguousarray(local, dtype=np.float64).reshape(-1)
        out = np.zeros((self.n_ranks, a.size))
        self._check(self._L.mpmc_comm_allgather_f64(self._h, _dp(a), a.size, _dp(out)))
        return out

    def gather_beads(self, local: np.ndarray) -> np.ndarray:
        """(n_local, stride) of this rank's beads (local-slot order) -> (P, stride) in bead order; bead s = rank s % n_ranks, slot s // n_ranks."""
        a = np.ascontiguousarray(local, dtype=np.float64)
        n_local = a.shape[0]
        a2 = a.reshape(n_local, -1)
        out = np.zeros((n_local * self.n_ranks, a2.shape[1]))
        self._check(self._L.mpmc_pi_gather_beads(self._h, _dp(a2), n_local, a2.shape[1], _dp(out)))
        return out.reshape((n_local * self.n_ranks,) + a.shape[1:])

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.mpmc_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pi_finish(sums4_global: np.ndarray, P: int):
    s = np.ascontiguousarray(sums4_global, dtype=np.float64)
    obs = np.zeros(4)
    v = lib().mpmc_pi_finish(_dp(s), int(P), _dp(obs))
    return v, obs


def pi_chain_mass_length2(coms: np.ndarray, mol_mass: np.ndarray, movable: Optional[np.ndarray] = None) -> float:
    """SimulationControl::PI_chain_mass_length2_ENTIRE_SYSTEM (reference PathIntegral.cpp:851-965).
    coms: (P, n_molecules, 3) centres of mass of the P images; host arithmetic inside libmpmc_energy.so."""
    c = np.ascontiguousarray(coms, dtype=np.float64)
    P, nmol, _ = c.shape
    m = np.ascontiguousarray(mol_mass, dtype=np.float64)
    mv = None if movable is None else np.ascontiguousarray(movable, dtype=np.int32)
    return float(lib().mpmc_pi_chain_mass_length2(P, nmol, _dp(c), _dp(m), _ip(mv)))


def pi_kinetic(chain_mass_len2: float, N: float, P: int, temperature: float, orient_mu_len2: float = 0.0) -> float:
    """SimulationControl::PI_calculate_kinetic (reference PathIntegral.cpp:806-824), Kelvin."""
    return float(lib().mpmc_pi_kinetic(float(chain_mass_len2), float(orient_mu_len2), float(N), int(P), float(temperature)))
