#!/bin/bash
# per-kernel register / scratch / LDS / occupancy figures for csrc/kernels.hip, csrc/light_general.hip, then csrc/cube_mips.hip, csrc/cube_prefilter.hip, csrc/cube_sh.hip, csrc/env_brdf.hip, csrc/sky.hip, csrc/post_aa.hip, csrc/fog.hip, csrc/ssr.hip, csrc/ssr_gloss.hip, csrc/ssr_pyramid.hip, csrc/dof.hip, csrc/decal.hip, csrc/bloom.hip, csrc/taa.hip, csrc/taa_upscale.hip, csrc/motion_blur.hip csrc/grade.hip (its LDS is sized at the launch: 4 N^3 bytes) and csrc/sharpen.hip (run from the repo root)
for f in kernels light_general cube_mips cube_prefilter cube_sh env_brdf sky post_aa fog ssr ssr_gloss ssr_pyramid dof decal bloom taa taa_upscale motion_blur grade sharpen; do
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -I include -I crychic_renderer_amd/csrc -c crychic_renderer_amd/csrc/$f.hip -o /tmp/k.o -Rpass-analysis=kernel-resource-usage 2>&1 \
 | grep remark | sed -E 's/.*remark: +//; s/ \[-Rpass.*//' | awk '/Function Name/{printf "\n%s ", $0; next}{printf "| %s ", $0}END{print ""}' | sed -E 's/\| (Bytes|Dynamic|Uses)[^|]*//g; s/_ZN3cry//'
done
