#!/bin/bash
# tools/make_pi_gs_ranked_golden.sh -- makes tests/golden/pi_gs_ranked: the path-integral case tests/golden/pi_gs with `polar_gs on` replaced
# by `polar_gs_ranked on` (job name "gsranked"), run by the UNMODIFIED reference executable (oracle/_ref/mpmcxx, built in place by
# `make -C oracle ref`) with -P 4.  Needs the reference tree (build container only).  What is kept is data: the input, the energy / dipole /
# field traces, the final averages block and the final bead geometries, as tools/make_pi_relax_golden.sh keeps them for pi_relax.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
G=$here/../tests/golden
BIN=$here/../oracle/_ref/mpmcxx
mkdir -p "$G/pi_gs_ranked"
sed -e 's/^job_name gs$/job_name gsranked/' -e 's/^polar_gs on$/polar_gs_ranked on/' "$G/pi_gs/input.in" >"$G/pi_gs_ranked/input.in"
grep -q '^polar_gs_ranked on$' "$G/pi_gs_ranked/input.in" && grep -q '^job_name gsranked$' "$G/pi_gs_ranked/input.in" && ! grep -q '^polar_gs ' "$G/pi_gs_ranked/input.in"
cp "$G/pi_gs/ion27.pqr" "$G/pi_gs_ranked/ion27.pqr"
d=$(mktemp -d)
cp "$G/pi_gs_ranked/input.in" "$G/pi_gs_ranked/ion27.pqr" "$d"/
(cd "$d" && "$BIN" -P 4 input.in >stock.log 2>&1)
cp "$d/gsranked.energy.dat" "$G/pi_gs_ranked/golden_energy.dat"
for f in "$d"/gsranked.final-*.pqr; do cp "$f" "$G/pi_gs_ranked/golden_${f##*/gsranked.}"; done
for k in dipole field; do [ -s "$d/gsranked.$k.dat" ] && cp "$d/gsranked.$k.dat" "$G/pi_gs_ranked/golden_$k.dat"; done
grep -E '^OUTPUT: (AR =|total energy|kinetic energy|polarization energy)' "$d/stock.log" | tail -12 >"$G/pi_gs_ranked/golden_final_averages.txt"
echo "pi_gs_ranked: $(grep -vc '^#' "$G/pi_gs_ranked/golden_energy.dat") energy rows"
rm -rf "$d"
