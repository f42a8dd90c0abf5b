"""CPU: cavity_autoreject -- the numpy restatement (tests/cavity_autoreject_ref.py) against the reference's goldens
(tests/golden/autoreject_cases.json, tools/make_autoreject_golden.py), the readers, the header and the ctypes mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cavity_autoreject_ref as R
import util
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import energy, gen_box, pqr

MAXVALUE = 1.0e40
CASES = sorted(R.cases())


def test_the_cases_the_goldens_were_built_for_are_all_there():
    c = R.cases()
    assert {"ion216_polar_s10", "ion216_polar_s08", "water64_polar_s07", "water64_polar_s09", "water64_polar_s10", "ion216_frozen_nopol_s10",
            "water64_polar_abs10", "ion216_frozen_nopol_abs05", "ion216_frozen_abs05", "ion216_triclinic_s10", "ion216_polar_rdm_b147wh_s10",
            "ion216_polar_rdm_drdwh_s10", "ion216_disp_s10", "ion216_disp_s09_rep100", "ion216_disp_s09", "abs_cell_abs10", "abs_face_abs10",
            "abs_face_both10"} == set(c)
    # the repulsion test of the disp-expansion term replaces pairs the sigma test at the same scale leaves alone
    assert c["ion216_disp_s09_rep100"]["result"]["lj_pairs"] > c["ion216_disp_s09"]["result"]["lj_pairs"] + 0.5e40
    # the figures measured on the reference
    assert c["ion216_polar_s10"]["result"]["rd"] == 1.5999999999999997e+41
    assert c["water64_polar_s09"]["result"]["rd"] == 9.2000000000000009e+41 and c["water64_polar_s10"]["result"]["rd"] == 1.5499999999999998e+42
    assert c["ion216_frozen_nopol_s10"]["result"]["rd"] == 1.4999999999999997e+41
    assert c["ion216_frozen_nopol_abs05"]["result"]["total"] == 1e40 and c["ion216_frozen_nopol_abs05"]["result"]["rd"] == -103316.23966526017
    for name in ("ion216_polar_s08", "water64_polar_s07", "water64_polar_abs10", "ion216_frozen_abs05"):  # no contact: the plain numbers
        assert c[name]["result"]["total"] == c[name]["plain"]["total"] == util.golden(c[name]["base"])["total"], name


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    atoms, basis, opts, case = R.load(name)
    g, plain = case["result"], case["plain"]
    rules, scale = R.rules_of(opts)
    c = R.restated(name)
    # the replaced pairs exactly; the absolute penalty exactly, the quirk of unmeasured frozen pairs included
    assert c["n_replaced"] == round(g["lj_pairs"] / MAXVALUE)
    if not rules & R.SIGMA:
        assert c["n_replaced"] == 0 and g["lj_pairs"] == plain["lj_pairs"] and g["rd"] == plain["rd"]
    penalty = MAXVALUE if c["n_absolute"] + c["n_unmeasured_frozen"] > 0 else 0.0
    assert (penalty > 0) == (g["total"] - g["rd"] > 0.5 * MAXVALUE)
    if name == "ion216_frozen_nopol_abs05":
        nf = int(np.sum(atoms["frozen"] != 0))  # (every 5th of 216 atoms frozen, one molecule each)
        assert nf > 40 and (c["n_absolute"], c["n_unmeasured_frozen"]) == (0, nf * (nf - 1) // 2)
    if name == "ion216_frozen_abs05":
        assert (c["n_absolute"], c["n_unmeasured_frozen"]) == (0, 0)
    if name.startswith("abs_"):
        assert c["n_absolute"] >= 1 and c["n_unmeasured_frozen"] == 0
    # rd and total within REL_TOL, from the contract: lj_pairs = S + n 1e40 with S the unpenalised pair sum (the reference's own)
    form = "lj" if not (opts.get("dreiding") or opts.get("lj_buffered_14_7")) else "other"
    mine = R.penalised({"lj_pairs": plain["lj_pairs"], "lrc_pair": plain["rd"] - plain["lj_pairs"] if form == "lj" else 0.0, "lrc_self": 0.0,
                        "coulombic_energy": plain["es"], "polarization_energy": plain["polar"]}, c, form)
    assert util.close(mine["rd_energy"], g["rd"]) and util.close(mine["lj_pairs"], g["lj_pairs"]), (name, mine, g["rd"])
    assert util.close(mine["returned_energy"], g["total"]), (name, mine["returned_energy"], g["total"])
    assert mine["absolute_penalty"] == penalty


def test_planted_pairs_of_the_absolute_boxes():
    """the moved molecule's H sits 0.8 A from another molecule's O: in the cell, and through the periodic image"""
    for name, face in (("abs_cell_abs10", False), ("abs_face_abs10", True)):
        atoms, basis, opts, _ = R.load(name)
        pairs = R.restated(name)["absolute_pairs"]
        d = [np.linalg.norm(atoms["pos"][i] - atoms["pos"][j]) for i, j in pairs]
        assert pairs and all(atoms["mol_id"][i] != atoms["mol_id"][j] for i, j in pairs)
        if face:
            assert min(d) > 10.0  # (only the image is close)
        else:
            assert abs(min(d) - 0.8) < 1e-5


def test_python_reader_keeps_refusing_and_the_options_carry_the_keywords(tmp_path):
    assert "cavity_autoreject" in pqr.UNSUPPORTED_ON and "cavity_autoreject_absolute" in pqr.UNSUPPORTED_ON
    inp, _ = gen_box.materialize("water64_polar", str(tmp_path))
    with open(inp, "a") as f:
        f.write("cavity_autoreject_absolute on\n")
    with pytest.raises(NotImplementedError):
        pqr.read_input(inp)
    assert energy.autoreject_of({"cavity_autoreject": 1, "cavity_autoreject_scale": 0.7}) == (1, 0.7, 0.0)
    assert energy.autoreject_of({"cavity_autoreject_absolute": "on", "cavity_autoreject": 0, "cavity_autoreject_scale": 1.0,
                                 "cavity_autoreject_repulsion": 2.5}) == (2, 1.0, 2.5)
    assert energy.autoreject_of({}) == (0, 0.0, 0.0) and set(energy.AUTOREJECT_KEYS) == set(R.KEYS)


def _build_check(tmp_path):
    lib = os.path.dirname(mbuild.LIB)
    mbuild.build_library()
    exe = str(tmp_path / "cavity_autoreject_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(util.ROOT, "include"),
                           os.path.join(util.ROOT, "tests", "cpp", "cavity_autoreject_check.cpp"), "-L", lib, "-lmpmc_energy", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_reader_takes_the_four_keywords(tmp_path):
    exe = _build_check(tmp_path)
    inp, _ = gen_box.materialize("water64_polar", str(tmp_path))
    txt = open(inp).read()

    def run(text):
        p = tmp_path / "case.in"
        p.write_text(text)
        out = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split("\n")[0]

    assert run(txt) == "read 0 0 0 0 0 0"
    assert run(txt + "cavity_autoreject on\ncavity_autoreject_scale 0.7\n") == "read 1 0 0.69999999999999996 0 1 1"
    assert run(txt + "cavity_autoreject_absolute on\ncavity_autoreject_scale 1.0\ncavity_autoreject_repulsion 2.5\n") == "read 0 1 1 2.5 2 1"
    assert run(txt + "cavity_autoreject on\ncavity_autoreject_absolute on\ncavity_autoreject_scale 0.5\n") == "read 1 1 0.5 0 3 1"
    assert run(txt + "cavity_autoreject off\ncavity_autoreject_scale 0.5\n") == "read 0 0 0.5 0 0 0"
    # a scale outside (0, 1] with a rule on is the reader's invalid input (SimulationControl.cpp:2139-2154)
    for bad in ("0", "1.5", "-0.2"):
        assert run(txt + f"cavity_autoreject on\ncavity_autoreject_scale {bad}\n") == "read thrown 3000"
    assert run(txt + "cavity_autoreject_absolute on\n") == "read thrown 3000"  # (the reference's default scale is 0)


def test_ctypes_mirror_has_the_size_of_the_header_struct(tmp_path):
    exe = _build_check(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["sizeof", str(C.sizeof(energy.AutorejectInfo))], out.stdout
    h = open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read()
    body = re.search(r"struct mpmc_cavity_autoreject_info \{(.*?)\};", h, flags=re.S).group(1)
    names = [n for decl in re.findall(r"^\s*(?:int32_t|int64_t|double)\s+([^;]+);", body, flags=re.M) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [f for f, _ in energy.AutorejectInfo._fields_]


def test_header_declares_the_entry_points_and_the_library_has_them():
    h = open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read()
    assert "#define MPMC_ABI_VERSION 6" in h and "#define MPMC_AUTOREJECT_SIGMA 1" in h and "#define MPMC_AUTOREJECT_ABSOLUTE 2" in h
    assert re.search(r"int mpmc_set_cavity_autoreject\(mpmc_ctx \*ctx, int rules[^)]*, double scale, double repulsion\);", h)
    assert re.search(r"int mpmc_cavity_autoreject_info\(mpmc_ctx \*ctx, struct mpmc_cavity_autoreject_info \*out\);", h)
    assert re.search(r"#define\s+MPMC_FLAG_CAVITY_AUTOREJECT\s+\(1ull << 16\)", h)
    assert "cavity_autoreject stays refused" not in h and "sigma_ij / 300" in h  # (a replaced pair's own energy stays in S: said in the header)
    L = energy.lib()
    assert hasattr(L, "mpmc_set_cavity_autoreject") and hasattr(L, "mpmc_cavity_autoreject_info") and hasattr(L, "mpmc_insert_candidates_contacts")
    assert re.search(r"int mpmc_insert_candidates_contacts\(mpmc_ctx \*ctx, int n_cand, int64_t \*n_replaced[^,]*, int64_t \*n_absolute[^)]*\);", h)
    assert L.mpmc_insert_candidates_contacts(None, 1, None, None) == -3
    assert "kernels_contact.hip" in mbuild.SOURCES
    assert L.mpmc_set_cavity_autoreject(None, 1, 0.5, 0.0) == -3  # (a null context: MPMC_ERR_ARG)


def test_restatement_on_a_hand_made_box():
    """two single-atom molecules and one two-atom molecule in a cubic 20 A cell: each rule counts what the contract says"""
    pos = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [9.7, 0.0, 0.0], [-9.7, 0.0, 0.0]])  # (atoms 2 and 3: 0.6 A apart through the face)
    atoms = {"pos": pos, "charge": np.zeros(4), "polarizability": np.zeros(4), "epsilon": np.array([100.0, 100.0, 0.0, 50.0]),
             "sigma": np.array([3.4, 3.0, 0.0, 2.0]), "mass": np.ones(4), "mol_id": np.array([0, 1, 2, 3], np.int32),
             "frozen": np.array([0, 0, 1, 1], np.int32), "has_disp": np.zeros(4, np.int32)}
    basis = np.eye(3) * 20.0
    c = R.counts(atoms, basis, {"polarization": 1}, R.SIGMA | R.ABSOLUTE, 1.0)
    assert c["replaced_pairs"] == [(0, 1)]  # 3.0 < (3.4 + 3.0) / 2; the pair (2, 3) is null and frozen
    assert c["absolute_pairs"] == [(2, 3)] and c["n_unmeasured_frozen"] == 0  # measured with polarization on: 0.6 A through the image
    c = R.counts(atoms, basis, {"polarization": 0}, R.SIGMA | R.ABSOLUTE, 1.0)
    assert c["absolute_pairs"] == [] and c["n_unmeasured_frozen"] == 1  # not measured without: the quirk pair
    c = R.counts(atoms, basis, {"polarization": 0}, R.SIGMA, 0.9)
    assert c["n_replaced"] == 0 and c["n_absolute"] == 0 and c["n_unmeasured_frozen"] == 0  # 3.0 > 0.9 * 3.2
    r = R.penalised({"lj_pairs": -5.0, "lrc_pair": -1.0, "lrc_self": -0.5, "coulombic_energy": 2.0, "polarization_energy": -0.25},
                    {"n_replaced": 2, "n_absolute": 0, "n_unmeasured_frozen": 1})
    assert r["lj_pairs"] == -5.0 + 2e40 and r["rd_energy"] == ((-5.0 + 2e40) - 1.0) - 0.5 and r["returned_energy"] == r["energy"] + 1e40
