#!/bin/sh
# Retired: HX_PIPE_ABL became constants in round 6, so this script built (or compared) identical libraries.
echo "build_diag.sh: HX_PIPE_ABL left the sources in round 6; use tools/build_variant.sh --switches hx_analysis.hip abl<N> \"-DHX_DIAG -DHX_PIPE_ABL=<N>\"" >&2
exit 1
