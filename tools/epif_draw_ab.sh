#!/bin/bash
# The moved sample-table draw (epif_draw_table in csrc/epif_dev.hpp, called by k_epif_gather and k_minit_gather) against the
# epifilter.hip of another revision, in one session, alternating: ov2_epipolar_filter_batch at 4096 items
# (tools/epifilter_time.py) and the ov2_btracker_track_mono_resident step at 4096 sequences (tools/resident_step_time.py).
#   tools/epif_draw_ab.sh build <git revision>   the variant: that revision's epifilter.hip compiled against that revision's headers,
#                                                linked with the objects of this tree -> build_var/epif_ab/libov2slam_hip.so
#   tools/epif_draw_ab.sh run [rounds] [outdir]  this, variant, this, variant, ...; one JSON file per run under outdir
#                                                (default profiles/monoinit_ab)
# "Not slower" is read as the README rows of f20 - f24 read it: the quartile ranges of neighbouring runs overlap.
set -eo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
VAR=$ROOT/build_var/epif_ab
case "$1" in
build)
    REV=${2:?a git revision}
    make -C $ROOT/ov2slam_amd/csrc -j8 > /dev/null
    rm -rf $VAR; mkdir -p $VAR/src
    git -C $ROOT archive $REV ov2slam_amd/csrc include | tar -x -C $VAR/src
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function \
        -c $VAR/src/ov2slam_amd/csrc/epifilter.hip -o $VAR/epifilter.o
    OBJS=$(ls $ROOT/ov2slam_amd/csrc/*.o | grep -v "/epifilter.o")
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $VAR/libov2slam_hip.so $OBJS $VAR/epifilter.o
    rm -rf $VAR/src $VAR/epifilter.o
    echo $VAR/libov2slam_hip.so
    ;;
run)
    ROUNDS=${2:-3}; OUT=${3:-$ROOT/profiles/monoinit_ab}
    test -f $VAR/libov2slam_hip.so || { echo "no variant: tools/epif_draw_ab.sh build <revision> first"; exit 1; }
    mkdir -p $OUT
    cd $ROOT
    for i in $(seq 1 $ROUNDS); do
        for side in this variant; do
            LIB=$ROOT/ov2slam_amd/libov2slam_hip.so; [ $side = variant ] && LIB=$VAR/libov2slam_hip.so
            OV2SLAM_HIP_LIB=$LIB timeout -k 10 300 python tools/epifilter_time.py 5 $OUT/epifilter_${side}_$i.json > /dev/null
            OV2SLAM_HIP_LIB=$LIB timeout -k 10 300 python tools/resident_step_time.py 4096 8 1 --forms resident --out $OUT/step_${side}_$i.json > /dev/null
            echo "round $i $side done"
        done
    done
    ;;
*)
    echo "usage: tools/epif_draw_ab.sh build <revision> | run [rounds] [outdir]"; exit 2
    ;;
esac
