#!/bin/bash
# A/B helper: ab/<name>/libdsd2dxd_amd.so = the tree's library with SOME translation units recompiled with extra hipcc flags
# (make the tree first).  Select it at run time with D2D_AMD_LIB=$PWD/ab/<name>/libdsd2dxd_amd.so (dsd2dxd_amd/_capi.py,
# development only; bench.py names such a library in its line and cites no counter traffic for it).
#   tools/ab_build.sh <name> <target> [flags...]     target: mx | mxm | mfma3 | kernels | px
#     mx       the fp6 kernel, E_M32 shape only (-DD2D_MX_DEV: the dispatcher with unit 0, and the shape's gain unit):
#              -DD2D_MX_ABL=<mask> -DD2D_MX_STAMPS=1 -DD2D_MX_G4=<groups> -DD2D_MX_NOFLAT=1 -DD2D_MX_NRES=<resident fragments> -DD2D_MX_RESIDENT=0 -DD2D_MX_FEED=0
#     mxm      the fp6 kernel, the three-pairs-per-wave unit of the E_M32 shape: -DD2D_MX_ABL=<mask>
#     mfma3    the pipelined int8 kernel, E_M8 shape only (-DD2D_M3_DEV: the dispatcher with unit 0): -DD2D_M3_ABL=<mask> -DD2D_M3_STAMPS=1
#     kernels  d2d_kernels.hip (LUT, resampler, de-interleave, noise shaping)
#     px       the direct polyphase kernel, every unit:              -DD2D_PX_ABL=<mask> -DD2D_PX_THREADS=768
# Every other object comes from the tree; the units are the rows of D2D_MX_UNIT_LIST (d2d_mx.h) / D2D_PX_UNIT_LIST (d2d_px.h) / D2D_M3_UNIT_LIST (d2d_m3.h).
set -e
NAME=$1; TARGET=$2; shift; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd); CS=$ROOT/dsd2dxd_amd/csrc; O=$ROOT/ab/$NAME
mkdir -p $O
HIPCC=/opt/rocm/bin/hipcc
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result -I$CS -I$ROOT/filters"
MX_UNITS=$(sed -n 's/^MX_UNITS = //p' $CS/Makefile); PX_UNITS=$(sed -n 's/^PX_UNITS = //p' $CS/Makefile); M3_UNITS=$(sed -n 's/^M3_UNITS = //p' $CS/Makefile)
COUNTS="-DD2D_MX_UNITS=$MX_UNITS -DD2D_PX_UNITS=$PX_UNITS -DD2D_M3_UNITS=$M3_UNITS"
mx_unit_of() { grep -o "X([0-9]*, $1)" $CS/d2d_mx.h | sed 's/X(\([0-9]*\),.*/\1/'; }     # the unit of the row "MB, NT, flavour, NPR"
mx_unit() { $HIPCC $FL -DD2D_MX_UNIT=$1 "${@:2}" -c $CS/d2d_mx_unit.hip -o $O/d2d_mx_unit$1.o; }
DEV=       # the flag that leaves units out of a dispatcher: the route unit's lookups need it too, or they name units the dispatcher does not hold
case $TARGET in
  mx)      DEV=-DD2D_MX_DEV=1
           $HIPCC $FL $COUNTS $DEV "$@" -c $CS/d2d_kernels_mx.hip -o $O/d2d_kernels_mx.o &
           mx_unit $(mx_unit_of "4, 560, MX_GAIN, 1") "$@"; wait ;;
  mxm)     mx_unit $(mx_unit_of "4, 560, MX_INT, 3") "$@" ;;
  mfma3)   DEV=-DD2D_M3_DEV=1
           $HIPCC $FL $COUNTS $DEV "$@" -c $CS/d2d_kernels_mfma3.hip -o $O/d2d_kernels_mfma3.o ;;
  px)      $HIPCC $FL $COUNTS "$@" -c $CS/d2d_kernels_px.hip -o $O/d2d_kernels_px.o &
           for i in $(seq 1 $((PX_UNITS - 1))); do $HIPCC $FL -DD2D_PX_UNIT=$i "$@" -c $CS/d2d_px_unit.hip -o $O/d2d_px_unit$i.o & done; wait ;;
  kernels) $HIPCC $FL "$@" -c $CS/d2d_kernels.hip -o $O/d2d_kernels.o ;;
  *) echo "target: mx | mxm | mfma3 | kernels | px"; exit 2 ;;
esac
# (the engine sees the geometry macros too: groups per column name the kernel)
$HIPCC $FL -x hip "$@" -c $CS/d2d_engine.cpp -o $O/d2d_engine.o
# ... and so do the choice of the route and the launch plans (the lists of kept units, the groups per column, the threads per block, the resident fragments)
g++ -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$CS -I$ROOT/filters $DEV "$@" -c $CS/d2d_route.cpp -o $O/d2d_route.o
# the tree's objects, each replaced by the one just built where there is one
OBJS=
for n in d2d_kernels d2d_kernels_rs d2d_kernels_mfma d2d_kernels_mfma2 d2d_engine d2d_tables d2d_route \
         d2d_kernels_mfma3 $(for i in $(seq 1 $((M3_UNITS - 1))); do echo d2d_m3_unit$i; done) \
         d2d_kernels_mx $(for i in $(seq 1 $((MX_UNITS - 1))); do echo d2d_mx_unit$i; done) \
         d2d_kernels_px $(for i in $(seq 1 $((PX_UNITS - 1))); do echo d2d_px_unit$i; done) \
         flac/d2d_flac flac/d2d_flac_verify flac/d2d_flac_md5 flac/d2d_flac_host flac/d2d_flac_stream \
         loud/d2d_loud loud/d2d_true_peak loud/d2d_loud_host \
         host/dsd_reader host/pcm_sink host/id3_tag host/rdsd2pcm host/rdsd2pcm_c; do
  if [ -f $O/$(basename $n).o ]; then OBJS="$OBJS $O/$(basename $n).o"; else OBJS="$OBJS $CS/$n.o"; fi
done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $O/libdsd2dxd_amd.so $OBJS -lpthread
echo built ab/$NAME
