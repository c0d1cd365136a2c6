#!/bin/sh
# Retired: HX_FFT_ABL became constants in round 6, so this script built (or compared) identical libraries.
echo "fft_ablate.sh: HX_FFT_ABL left the sources in round 6; use tools/build_variant.sh --switches hx_sht.hip fa<bits> \"-DHX_FFT_ABL=<bits>\"" >&2
exit 1
