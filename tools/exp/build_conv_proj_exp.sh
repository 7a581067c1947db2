#!/bin/bash
# usage (build container): tools/exp/build_conv_proj_exp.sh <tag> <bits>
# Links tools/exp/ab/lib_<tag>.so = the in-tree library with csrc/conv_proj.hip recompiled from a scratch copy that carries
# tools/exp/conv_proj_exp_hooks.patch and -DARREAU_CP_EXP=<bits> (timing-only: each bit removes one part of the message kernel's
# slot step, the results are WRONG on purpose; the bits are listed at the top of the patched source).  Prints the kernel's
# register and scratch figures, so that a variant that changed more than its one part (a spill) is seen before it is timed.
set -e
tag=$1; bits=$2
cd "$(dirname "$0")/../.."
root=$(pwd)
csrc=arreau_amd/csrc
tmp=$(mktemp -d /tmp/arreau_cp_exp_XXXXXX)
mkdir -p tools/exp/ab "$tmp/arreau_amd"
python -m arreau_amd.build >/dev/null 2>&1
cp -r $csrc "$tmp/arreau_amd/" && cp -r include "$tmp/"
(cd "$tmp" && patch -p1 -s --fuzz=0 < "$root/tools/exp/conv_proj_exp_hooks.patch")  # (a hunk that no longer fits exactly fails the build)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++20 -fPIC -Wno-inline-asm -Wno-unused-but-set-variable -Wno-misleading-indentation \
    -Wno-uninitialized -ffp-contract=on -DARREAU_CP_EXP=$bits -Rpass-analysis=kernel-resource-usage \
    -c "$tmp/$csrc/conv_proj.hip" -o "$tmp/conv_proj.o" 2> "$tmp/remarks.txt"
grep -A12 'Function Name: .*conv_proj_kernelILi128ELi256ELi4ELb1ELb1E' "$tmp/remarks.txt" | grep -E 'VGPRs:|ScratchSize' | sed "s/^.*remark: [^ ]* */  $tag: /"
objs=""
for o in $csrc/*.o; do
  if [ "$(basename $o)" = conv_proj.o ]; then objs="$objs $tmp/conv_proj.o"; else objs="$objs $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/exp/ab/lib_$tag.so $objs
rm -rf "$tmp"
echo built tools/exp/ab/lib_$tag.so
