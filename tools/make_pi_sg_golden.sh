#!/bin/bash
# tools/make_pi_sg_golden.sh -- makes tests/golden/pi_sg: the path-integral case tests/golden/pi_gs as 27 single-site H2 molecules under the
# Silvera-Goldman potential (job name "sg": the polarization and Ewald lines leave, `sg on` comes; the atoms keep their places and become
# uncharged H2 sites of mass 2.016), same step count and seed, run by the UNMODIFIED reference executable (oracle/_ref/mpmcxx, built in
# place by `make -C oracle ref`) with -P 4.  Needs the reference tree (build container only).  What is kept is data: the input, the energy
# trace, the final averages block and the final bead geometries, as oracle/make_pi_golden.sh keeps them for the other pi_* cases.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
G=$here/../tests/golden
BIN=$here/../oracle/_ref/mpmcxx
mkdir -p "$G/pi_sg"
sed -e 's/^job_name gs$/job_name sg/' -e '/^polarization /d' -e '/^polar_/d' -e '/^ewald_kmax /d' -e 's/^pqr_input ion27.pqr$/sg on\npqr_input h2_27.pqr/' \
	"$G/pi_gs/input.in" >"$G/pi_sg/input.in"
grep -q '^sg on$' "$G/pi_sg/input.in" && ! grep -q '^polar' "$G/pi_sg/input.in"
awk '$1 == "ATOM" { printf "ATOM %6d %-4s %-4s %s %6d %12.6f %12.6f %12.6f %9.5f %9.5f %8.5f %10.5f %8.5f 0.00000 0.00000\n", $2, "H2G", "H2", $5, $6, $7, $8, $9, 2.016, 0, 0, 34.2, 2.96 } END { print "END" }' \
	"$G/pi_gs/ion27.pqr" >"$G/pi_sg/h2_27.pqr"
[ "$(grep -c "^ATOM" "$G/pi_sg/h2_27.pqr")" -eq 27 ]
d=$(mktemp -d)
cp "$G/pi_sg/input.in" "$G/pi_sg/h2_27.pqr" "$d"/
(cd "$d" && "$BIN" -P 4 input.in >stock.log 2>&1)
cp "$d/sg.energy.dat" "$G/pi_sg/golden_energy.dat"
for f in "$d"/sg.final-*.pqr; do cp "$f" "$G/pi_sg/golden_${f##*/sg.}"; done
grep -E '^OUTPUT: (AR =|total energy|kinetic energy|polarization energy)' "$d/stock.log" | tail -12 >"$G/pi_sg/golden_final_averages.txt"
echo "pi_sg: $(grep -vc '^#' "$G/pi_sg/golden_energy.dat") energy rows"
rm -rf "$d"
