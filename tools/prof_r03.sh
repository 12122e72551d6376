set -x
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; O=${O:-prof_out/r03}; mkdir -p $O
# 1. kernel trace of the headline command (short)
rocprofv3 --kernel-trace --stats -d $O/kt -- python bench.py --full --steps 20 --warmup 5 --no-variants --no-cpu-baseline > $O/kt_bench.json 2> $O/kt.log
DB=$(find $O/kt -name "*results.db" | head -1); python tools/rocpd_stats.py $DB $O/kernel_stats_bench.md | head -25
# 2. PMC passes (separate; kernel-trace only beside --pmc)
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $c -d $O/pmc_$c -- python bench.py --full --steps 8 --warmup 3 --no-variants --no-cpu-baseline --prof-rounds 0 > /dev/null 2> $O/pmc_$c.log
  DB=$(find $O/pmc_$c -name "*results.db" | head -1); python tools/rocpd_pmc.py $DB > $O/pmc_$c.txt; grep -E "ppo_update_persistent|disc_fb|disc_fwd|disc_bwd|disc_reduce|ia_gemm_kernelILi2ELi2ELi1ELi1ELi2|disc_assemble|rn_merge_seq" $O/pmc_$c.txt | cut -c1-60,92-
done
# 3. variants: default 32x32 discriminator, tuned GAIL verbatim
for v in P_disc32 T_gail_half_cheetah_tuned_verbatim P_gp10; do
  rocprofv3 --kernel-trace --stats -d $O/kt_$v -- python tools/variant_profile.py $v 8 > $O/kt_$v.log 2>&1
  DB=$(find $O/kt_$v -name "*results.db" | head -1); python tools/rocpd_stats.py $DB $O/kernel_stats_$v.md | head -12
done
find $O -name "*.db" -size +20M -delete; du -sh $O
