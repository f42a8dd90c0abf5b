"""CPU side of the rd model (mpmc_set_rd_model: Waldman-Hagler / Halgren / C6 mixing, buffered 14-7 and DREIDING): the numpy restatement
against the reference's goldens, the host build of the pair functions of csrc/pair_math.h (plain and under the sanitizers), the fixtures,
the readers, the drivers, the header and the gfx950 code object of kernels_rd_model.hip."""
import os
import re
import subprocess

import numpy as np
import pytest

import rd_model_ref as R
import util
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import energy, gen_box, pqr
from test_cabi import _kernel_notes

EPS = np.finfo(float).eps
ALL = gen_box.RD_MODEL_FIXTURES
# the issue's cross-check of the generator: the reference's rd of the ion216_polar base under seven models
ISSUE_RD = {"ljwh": -36965.523085203466, "ljhal": -37412.13992751017, "ljc6": -37783.69955802282, "b147lb": -18461.132258025547,
            "b147hal": -18253.663148210846, "drdlb": -23045.419977203655}


def golden(name):
    return gen_box.rd_model_golden(util.GOLDEN, name)


@pytest.mark.parametrize("name", ALL)
def test_restatement_matches_reference_goldens(name):
    """rd, lj_pairs and lrc_pair within n_pairs EPS (mag + |lrc_pair|): the reference adds its pair list up naively in list order, the
    restatement in another order; the counts exactly"""
    g, r = golden(name), R.restated(name)
    bound = g["n_pairs"] * EPS * (r["mag"] + abs(g["lrc_pair"]))
    for ours, theirs in (("rd", "rd"), ("lj_pairs", "lj_pairs"), ("lrc_pair", "lrc_pair")):
        assert abs(r[ours] - g[theirs]) <= bound, (name, ours, r[ours], g[theirs], bound)
    assert r["n_lj_in_cutoff"] == g["n_lj_in_cutoff"], name
    if r["form"] != "lj":  # no corrections: rd is the pair sum (the harness's own lrc_self is not part of rd)
        assert g["lrc_pair"] == 0.0 and g["rd"] == g["lj_pairs"] and r["lrc_pair"] == 0.0 and r["lrc_self"] == 0.0 and r["rd"] == r["lj_pairs"], name
    else:  # the harness's lrc_self is lj_lrc_self of the atoms' own parameters: the restatement's, to the rounding of its sum
        assert abs(r["lrc_self"] - (g["lrc_self"] if R.load(name)[2]["rd_lrc"] else 0.0)) <= g["natoms"] * EPS * abs(g["lrc_self"]), name


def test_generator_reproduces_the_recorded_values():
    for tag, rd in ISSUE_RD.items():
        assert golden(f"ion216_polar_rdm_{tag}")["rd"] == rd, tag
    assert abs(golden("arkr_contact_rdm_drdlb")["rd"] - 6.63e41) < 0.005e41  # eps_ij 1e40 at 0.9 A


def test_three_species_under_the_default_model_give_the_recorded_plain_value():
    """the issue's seventh cross-check, the reference's rd of the three-species ion216_polar box with Lorentz-Berthelot and plain LJ: it pins
    the species assignment independently of the new mixing rules (the restatement's form and rule forced to the default)"""
    want = -38391.714054795724
    atoms, basis, opts = R.load("ion216_polar_rdm_ljwh")
    r = R.for_case(atoms, basis, opts, form="lj", rule="lb")
    n = len(atoms["sigma"])
    assert abs(r["rd"] - want) <= (n * (n - 1) // 2) * EPS * (r["mag"] + abs(r["lrc_pair"])), (r["rd"], want)


def test_two_atom_boxes_keep_the_pair_at_exactly_the_cutoff():
    """r = 5 exactly (3, 4, 0) is kept by every form; 1e-6 beyond it is dropped, 1e-6 inside it is kept"""
    for tag in ("ljwh", "b147lb", "drdlb"):
        eq, gt, lt = (R.restated(f"arkr_{t}_rdm_{tag}") for t in ("eq", "gt", "lt"))
        assert (eq["n_terms"], gt["n_terms"], lt["n_terms"]) == (1, 0, 1), tag
        assert eq["gap"] == 0.0 and golden(f"arkr_eq_rdm_{tag}")["cutoff"] == 5.0
        assert golden(f"arkr_eq_rdm_{tag}")["lj_pairs"] != 0.0 and golden(f"arkr_gt_rdm_{tag}")["lj_pairs"] == 0.0
        assert golden(f"arkr_lt_rdm_{tag}")["lj_pairs"] != 0.0
    c = R.restated("arkr_contact_rdm_drdlb")
    assert c["n_terms"] == 1 and c["lj_pairs"] > 6e41


@pytest.mark.parametrize("name", ALL)
def test_no_pair_sits_on_the_cutoff(name):
    """except in the deliberate exact-cutoff boxes no pair lies within 1e-9 relative of the cutoff: the counts are meaningful"""
    gap = R.restated(name)["gap"]
    if name.startswith("arkr_eq"):
        assert gap == 0.0, (name, gap)
    else:
        assert gap > 1e-9, (name, gap)


def test_every_fixture_has_a_golden_and_every_combination_appears():
    import json

    with open(os.path.join(util.GOLDEN, gen_box.RD_MODEL_GOLDEN)) as f:
        have = json.load(f)
    assert set(have) == set(ALL) and len(ALL) == len(set(ALL))
    seen = set()
    for name in ALL:
        form, rule = gen_box.rd_model_combo(name.rsplit("_rdm_", 1)[1])
        assert R.model_of(R.load(name)[2]) == (form, rule), name
        seen.add((form, rule))
    want = {(f, r) for f in R.FORMS for r in R.RULES} - {("lj", "lb")}
    assert seen == want, want - seen
    for b in ("ion216_polar", "water64_polar", "ion216_framework", "ion216_triclinic", "ion216_fh4_polar", "ion216_nolrc", "ion4000_polar", "arkr_eq",
              "arkr_gt", "arkr_lt", "arkr_contact"):
        assert any(n.startswith(b + "_rdm_") for n in ALL), b


@pytest.mark.parametrize("name", ALL)
def test_regenerated_boxes_are_the_ones_the_reference_evaluated(name):
    g = golden(name)
    rows, basis, opts = gen_box.fixture(name)
    assert g["fixture"] == name and g["natoms"] == len(rows)
    assert np.array_equal(np.asarray(g["basis"], dtype=np.float64).reshape(3, 3), np.asarray(basis, dtype=np.float64))
    assert not os.path.exists(os.path.join(util.GOLDEN, name + ".pqr")) and not os.path.exists(os.path.join(util.GOLDEN, name + ".json"))
    assert not any(isinstance(v, list) and k not in ("basis", "reciprocal_basis") for k, v in g.items())  # scalars only
    if not name.startswith("arkr_"):  # three species on the non-H rows, by atom_id % 5
        for r in rows:
            if r.atomtype != "H":
                assert (r.eps, r.sigma) == gen_box.RD_MODEL_SPECIES[{1: "B", 3: "B", 4: "C"}.get(r.atom_id % 5, "A")], (name, r.atom_id)
        assert len({(r.eps, r.sigma) for r in rows if r.atomtype != "H"}) == 3


def test_water_boxes_hold_unexcluded_pairs_with_a_mixed_sigma_of_zero():
    """the first H of every molecule carries a dispersion coefficient and no sigma: its pairs with other molecules are not excluded"""
    atoms, _, _ = R.load("water64_polar_rdm_b147hal")
    h = (atoms["sigma"] == 0.0) & (atoms["has_disp"] != 0)
    assert h.sum() == 64 and ((atoms["sigma"] == 0.0) & (atoms["has_disp"] == 0)).sum() == 64
    g, p = golden("water64_polar_rdm_b147hal"), util.golden("water64_polar")
    assert g["n_rd_excluded"] < p["n_rd_excluded"] and g["n_lj_in_cutoff"] > p["n_lj_in_cutoff"]
    i, j = np.nonzero(h)[0][:1], np.nonzero(atoms["sigma"] > 0.0)[0][-1:]
    for rule in R.RULES:
        sig, eps = R.mix(rule, atoms["sigma"][i], atoms["epsilon"][i], atoms["sigma"][j], atoms["epsilon"][j])
        assert (sig[0] == 0.0 or eps[0] == 0.0) and np.isfinite(sig[0]) and np.isfinite(eps[0]), rule
        for form in R.FORMS:
            assert R.pair_energy(form, sig, eps, np.array([3.0]))[0] == 0.0, (form, rule)


def test_terms_other_than_rd_are_the_plain_model_s():
    """es and polar of the reference do not depend on the model: the eleven ion216_polar goldens agree bit for bit"""
    first = golden(ALL[0])
    for name in ALL[1:11]:
        g = golden(name)
        for k in ("es", "polar", "es_real", "es_recip", "es_self", "n_lj_in_cutoff", "n_rd_excluded", "n_es_in_cutoff"):
            assert g[k] == first[k], (name, k)
        assert g["rd"] != first["rd"], name


# ---- the pair functions of pair_math.h on the host -------------------------------------------------------------------------------------
def _build_host_program(tmp_path, sanitize):
    exe = str(tmp_path / ("rd_model_check_san" if sanitize else "rd_model_check"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                          [os.path.join(util.ROOT, "tests", "cpp", "rd_model_check.cpp"), "-o", exe])
    return exe


def _ulps(a, b, scale):
    return np.abs(a - b) / np.spacing(np.abs(scale))


def test_host_program_agrees_with_the_restatement(tmp_path):
    """The MPMC_HD functions on a grid of (sigma_i, eps_i, sigma_j, eps_j, r) with sigma_j = 0, eps_j = 0 and r at 0.4 sigma_ij from both
    sides.  sigma_ij and eps_ij within 4 ulp of the restatement's; the energy within 4 ulp of the restatement's function of the program's
    own (sigma_ij, eps_ij, r), the ulp taken at the sum of the magnitudes of the function's two terms (it is their difference, and
    vanishes at the zero crossing: `mag` as everywhere in these tests).  A pair whose sigma_ij or eps_ij is 0 gives exactly 0, never a NaN.
    Measured: sigma 1 ulp, epsilon 4 ulp (C6), energy 0 (LJ), 4 (14-7), 4 (DREIDING)."""
    out = subprocess.run([_build_host_program(tmp_path, False)], capture_output=True, text=True, check=True, timeout=120).stdout
    a = np.array([[float(x) for x in ln.split()] for ln in out.strip().split("\n")])
    assert a.shape[1] == 10 and np.isfinite(a).all()
    for f, form in enumerate(R.FORMS):
        for m, rule in enumerate(R.RULES):
            s = a[(a[:, 0] == f) & (a[:, 1] == m)]
            assert len(s) > 300, (form, rule, len(s))
            sig, eps = R.mix(rule, s[:, 2], s[:, 3], s[:, 4], s[:, 5])
            assert np.array_equal(sig == 0.0, s[:, 7] == 0.0) and np.array_equal(eps == 0.0, s[:, 8] == 0.0), (form, rule)
            nz, ne = sig != 0.0, eps != 0.0
            assert _ulps(s[nz, 7], sig[nz], sig[nz]).max() <= 4 and _ulps(s[ne, 8], eps[ne], eps[ne]).max() <= 4, (form, rule)
            e = R.pair_energy(form, s[:, 7], s[:, 8], s[:, 6])
            mag = R.pair_mag(form, s[:, 7], s[:, 8], s[:, 6])
            null = (s[:, 7] == 0.0) | (s[:, 8] == 0.0)
            assert null.sum() >= 100 and np.all(s[null, 9] == 0.0) and np.all(e[null] == 0.0), (form, rule)
            assert _ulps(s[~null, 9], e[~null], mag[~null]).max() <= 4, (form, rule, _ulps(s[~null, 9], e[~null], mag[~null]).max())
            # end to end, against the restatement's own mixed parameters: sigma_ij and eps_ij may each be 4 ulp off, and the function's
            # terms depend on sigma_ij with a logarithmic derivative of at most k = 12 (LJ: (sigma / r)^12), 14 (14-7: the two seventh powers)
            # or max(6, 12 rho) (DREIDING: exp(12 (1 - rho)), rho^-6), so |dE| <= (4 + 4 + 4 k) ulp of mag.  The points within 8 ulp of the
            # contact threshold are left out here: there a 1-ulp sigma_ij decides between 1e40 and the exponential.
            e2, mag2 = R.pair_energy(form, sig, eps, s[:, 6]), R.pair_mag(form, sig, eps, s[:, 6])
            rho = np.where(sig > 0.0, s[:, 6] / np.where(sig > 0.0, sig, 1.0), 0.0)
            k = {"lj": 12.0, "b147": 14.0}.get(form, np.maximum(6.0, 12.0 * rho))
            away = ~null & ~((form == "drd") & (np.abs(s[:, 6] - 0.4 * sig) <= 8 * np.spacing(0.4 * sig)))
            worst = (_ulps(s[:, 9], e2, np.maximum(mag2, 1e-300)) / (8.0 + 4.0 * k))[away].max()
            assert worst <= 1.0, (form, rule, worst)
            if form == "drd":  # the contact branch is taken on both sides of 0.4 sigma_ij
                contact = ~null & (s[:, 6] < 0.4 * s[:, 7])
                assert contact.sum() >= 20 and np.all(s[contact, 9] > 1e40), (rule, contact.sum())
                assert (~null & (s[:, 6] == 0.4 * s[:, 7])).sum() >= 5 and np.all(np.abs(s[~null & ~contact, 9]) < 1e12)


def test_host_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined, run on its own"""
    exe = _build_host_program(tmp_path, True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    plain = subprocess.run([_build_host_program(tmp_path, False)], capture_output=True, text=True, check=True, timeout=120).stdout
    assert out.stdout == plain


# ---- readers, drivers, header, code object -----------------------------------------------------------------------------------------------
def test_python_reader_takes_the_keywords(tmp_path):
    _, _, o = R.load("ion216_polar_rdm_b147hal")
    assert o["lj_buffered_14_7"] == 1 and o["halgren_mixing"] == 1 and "dreiding" not in o
    assert energy.rd_model_of(o) == (energy.RD_FORM["lj_buffered_14_7"], energy.RD_MIX["halgren_mixing"])
    assert energy.rd_model_of(R.load("ion216_polar_rdm_b147lb")[2]) == (1, 0)  # lj_buffered_14_7 alone does not switch Halgren mixing on
    assert energy.rd_model_of({"dreiding": 1, "lj_buffered_14_7": 1, "c6_mixing": 1}) == (2, 3)  # dreiding wins
    _, _, o = util.load_fixture("ion216_polar")  # an input that names none of them loads as before
    assert not any(k in o for k in energy.RD_MODEL_KEYS) and energy.rd_model_of(o) == (0, 0)
    for k in energy.RD_MODEL_KEYS:
        assert k not in pqr.UNSUPPORTED_ON
    inp, _ = gen_box.materialize("ion216_polar_rdm_ljwh", str(tmp_path))
    txt = open(inp).read()
    case = tmp_path / "case.in"
    case.write_text(txt.replace("waldmanhagler on", "waldmanhagler off"))
    assert pqr.read_input(str(case))["options"]["waldmanhagler"] == 0
    for kw in ("cdvdw_exp_repulsion", "rd_anharmonic", "disp_expansion_mbvdw"):  # the other keywords of the two flag bits stay refused
        case.write_text(txt + kw + " on\n")
        with pytest.raises(NotImplementedError):
            pqr.read_input(str(case))
    case.write_text(txt + "c6_mixing on\n")  # two mixing rules
    with pytest.raises(ValueError):
        pqr.read_input(str(case))
    with pytest.raises(energy.MpmcError) as ei:
        energy.rd_model_of({"waldmanhagler": 1, "halgren_mixing": 1})
    assert ei.value.code == energy.ERR_INVALID_SETTING


def test_cpp_reader_and_drivers(tmp_path):
    """include/mpmc_io.hpp reads the five keywords into the facade's fields and raises no flag for them; it still raises the two flags for
    cdvdw_exp_repulsion and rd_anharmonic and refuses two mixing rules; the PI-NVT and Gibbs drivers refuse a System with a non-default
    model with 4004 before any evaluation"""
    lib = os.path.dirname(mbuild.LIB)
    mbuild.build_library()
    exe = str(tmp_path / "rd_model_facade_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(util.ROOT, "include"),
                           os.path.join(util.ROOT, "tests", "cpp", "rd_model_facade_check.cpp"), "-L", lib, "-lmpmc_energy", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    plain, _ = gen_box.materialize("ion216_polar", str(tmp_path))
    txt = open(plain).read()

    def run(text):
        p = tmp_path / "case.in"
        p.write_text(text)
        out = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split("\n")

    lines = run(txt)
    assert lines[0] == "read 0 0 0 0 0 form 0 mix 0 flags 0", lines
    assert lines[1:3] == ["pimc 4004", "gibbs 4004"], lines
    assert run(txt + "waldmanhagler on\n")[0] == "read 1 0 0 0 0 form 0 mix 1 flags 0"
    assert run(txt + "halgren_mixing on\nlj_buffered_14_7 on\n")[0] == "read 0 1 0 1 0 form 1 mix 2 flags 0"
    assert run(txt + "lj_buffered_14_7 on\n")[0] == "read 0 0 0 1 0 form 1 mix 0 flags 0"
    assert run(txt + "c6_mixing on\ndreiding on\nlj_buffered_14_7 on\n")[0] == "read 0 0 1 1 1 form 2 mix 3 flags 0"
    assert run(txt + "dreiding on\ndreiding off\n")[0] == "read 0 0 0 0 0 form 0 mix 0 flags 0"
    assert run(txt + "cdvdw_exp_repulsion on\n")[0] == f"read 0 0 0 0 0 form 0 mix 0 flags {1 << 14}"
    assert run(txt + "rd_anharmonic on\n")[0] == f"read 0 0 0 0 0 form 0 mix 0 flags {1 << 14}"
    assert run(txt + "cdvdw_sig_repulsion on\n")[0] == f"read 0 0 0 0 0 form 0 mix 0 flags {1 << 13}"
    assert run(txt + "waldmanhagler on\nhalgren_mixing on\n")[0] == "read thrown 3000"
    inp, _ = gen_box.materialize("ion216_polar_rdm_drdc6", str(tmp_path))
    assert run(open(inp).read())[0] == "read 0 0 1 0 1 form 2 mix 3 flags 0"


def test_header_keeps_abi_6_and_declares_the_entry_points():
    h = open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read()
    assert "#define MPMC_ABI_VERSION 6" in h and "#define MPMC_K_COUNT 8" in h
    for k, v in (("FORM_LJ", 0), ("FORM_BUFFERED_14_7", 1), ("FORM_DREIDING", 2), ("MIX_LB", 0), ("MIX_WALDMAN_HAGLER", 1), ("MIX_HALGREN", 2), ("MIX_C6", 3)):
        assert re.search(rf"#define\s+MPMC_RD_{k}\s+{v}\b", h), k
    assert re.search(r"int mpmc_set_rd_model\(mpmc_ctx \*ctx, int form, int mixing\);", h)
    assert re.search(r"int mpmc_rd_model_info\(mpmc_ctx \*ctx, struct mpmc_rd_model_info \*out\);", h)
    assert re.search(r"struct\s+mpmc_rd_model_info\s*\{[^}]*int32_t\s+form,\s*mixing;[^}]*int64_t\s+n_terms;[^}]*int64_t\s+n_tile_pairs;[^}]*"
                     r"int64_t\s+n_tile_pairs_skipped;[^}]*\};", h)
    assert re.search(r"#define\s+MPMC_FLAG_NON_LB_MIXING\s+\(1ull << 13\)", h) and re.search(r"#define\s+MPMC_FLAG_OTHER_RD\s+\(1ull << 14\)", h)
    assert "no force field uses any of these" in h
    assert C_sizeof_info() == 32
    L = energy.lib()
    assert hasattr(L, "mpmc_set_rd_model") and hasattr(L, "mpmc_rd_model_info")


def C_sizeof_info():
    import ctypes

    return ctypes.sizeof(energy.RdModelInfo)


def test_rd_model_fixtures_stay_out_of_the_other_lists():
    others = set(gen_box.SMALL_FIXTURES + gen_box.LARGE_FIXTURES + gen_box.THREE_BODY_FIXTURES + gen_box.DISP_FIXTURES + gen_box.WOLF_FIXTURES
                 + gen_box.DIRECT_FIXTURES + gen_box.RD_CRYSTAL_FIXTURES + gen_box.EWALD_FULL_FIXTURES + util.SMALL)
    assert not set(ALL) & others


def test_kernels_compile_for_gfx950_and_the_library_exports_the_entry_points():
    assert "kernels_rd_model.hip" in mbuild.SOURCES and "--offload-arch=gfx950" in mbuild.CFLAGS
    mbuild.build_library()
    assert os.path.getmtime(mbuild.LIB) >= os.path.getmtime(os.path.join(mbuild.CSRC, "kernels_rd_model.hip"))
    syms = subprocess.run(["nm", "-D", "--defined-only", mbuild.LIB], capture_output=True, text=True, check=True).stdout
    for s in ("mpmc_set_rd_model", "mpmc_rd_model_info"):
        assert re.search(r"\sT\s+" + s + r"\s", syms), s


def test_rd_model_kernels_need_no_scratch():
    """every instantiation of the two walks with the model's terms (cell shape x form x rule; rule alone for the correction) is in the gfx950 code object,
    spills nothing and keeps at least four waves per SIMD"""
    notes = _kernel_notes("kernels_rd_model.hip.o")
    full = [k for k in notes if "k_pair_term_sum" in k and "RdModelTermI" in k]  # (the shared walks of pair_term_walk.h with this file's terms)
    delta = [k for k in notes if "k_pair_term_delta" in k and "RdModelTermI" in k]
    lrc = [k for k in notes if "k_pair_term_sum" in k and "RdModelLrcTermI" in k]
    assert len(full) == 24 and len(delta) == 24 and len(lrc) == 4, (len(full), len(delta), len(lrc))
    for name in full + delta + lrc:
        meta = notes[name]
        assert meta["sgpr_spill_count"] == 0 and meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 128, (name, meta)
    for name in full:
        assert notes[name]["group_segment_fixed_size"] <= 8192, (name, notes[name])
