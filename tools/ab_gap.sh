#!/bin/sh
# Retired: HX_DUO_GAP became constants in round 6, so this script built (or compared) identical libraries.
echo "ab_gap.sh: HX_DUO_GAP left the sources in round 6; use tools/build_variant.sh --switches hx_analysis.hip g<N> \"-DHX_DUO_GAP=<N>\", then tools/ab_lib.sh default g<N> \"2 20\"" >&2
exit 1
