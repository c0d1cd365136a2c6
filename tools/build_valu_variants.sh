#!/bin/sh
# Retired: HX_VALU_WAVES and the other HX_VALU_* switches became constants in round 6, so this script built (or compared) identical libraries.
echo "build_valu_variants.sh: HX_VALU_WAVES and the other HX_VALU_* switches left the sources in round 6; use tools/build_variant.sh --switches hx_legendre_valu.hip <tag> \"-DHX_VALU_WAVES=2\"" >&2
exit 1
