#!/bin/bash
# tools/make_pi_relax_golden.sh -- makes tests/golden/pi_relax: the path-integral case tests/golden/pi_gs with `polar_gs on` replaced by
# `polar_esor on` / `polar_gamma 0.7` (job name "relax"), run by the UNMODIFIED reference executable (oracle/_ref/mpmcxx, built in place by
# `make -C oracle ref`) with -P 4.  Needs the reference tree (build container only).  What is kept is data: the input, the energy / dipole /
# field traces, the final averages block and the final bead geometries, as oracle/make_pi_golden.sh keeps them for the other pi_* cases.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
G=$here/../tests/golden
BIN=$here/../oracle/_ref/mpmcxx
mkdir -p "$G/pi_relax"
sed -e 's/^job_name gs$/job_name relax/' -e 's/^polar_gs on$/polar_esor on\npolar_gamma 0.7/' "$G/pi_gs/input.in" >"$G/pi_relax/input.in"
grep -q '^polar_esor on$' "$G/pi_relax/input.in" && grep -q '^polar_gamma 0.7$' "$G/pi_relax/input.in" && ! grep -q '^polar_gs' "$G/pi_relax/input.in"
cp "$G/pi_gs/ion27.pqr" "$G/pi_relax/ion27.pqr"
d=$(mktemp -d)
cp "$G/pi_relax/input.in" "$G/pi_relax/ion27.pqr" "$d"/
(cd "$d" && "$BIN" -P 4 input.in >stock.log 2>&1)
cp "$d/relax.energy.dat" "$G/pi_relax/golden_energy.dat"
for f in "$d"/relax.final-*.pqr; do cp "$f" "$G/pi_relax/golden_${f##*/relax.}"; done
for k in dipole field; do [ -s "$d/relax.$k.dat" ] && cp "$d/relax.$k.dat" "$G/pi_relax/golden_$k.dat"; done
grep -E '^OUTPUT: (AR =|total energy|kinetic energy|polarization energy)' "$d/stock.log" | tail -12 >"$G/pi_relax/golden_final_averages.txt"
echo "pi_relax: $(grep -vc '^#' "$G/pi_relax/golden_energy.dat") energy rows"
rm -rf "$d"
