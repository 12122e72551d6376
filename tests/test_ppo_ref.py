"""The float64 PPO reference of `tests/ppo_ref.py`, validated and measured on the CPU (no GPU, no HIP library).

For every case of `tests/ppo_ref.py` (all cases of tests/test_ppo_gradient_gpu.py):
  * validation: the float64 reference against `oracle.sb3_restated.PPO.train` itself, run in float32 on the same policy
    (`_oracle_policy`), the same buffer and the same `np.random.seed(123)` permutation -- the raw gradient of every step
    (read where `clip_grad_norm_` is called), the norm it returns, the optimiser's exp_avg and exp_avg_sq, the parameters,
    the logged statistics and the feature norm's state; clip_fraction and the norm's count exactly;
  * guards: `ppo_ref.assert_guards` (ratio margin, clipped norm, block scale) holds; each case's seed was picked by
    `python -m tests.test_ppo_ref seeds` so that it does;
  * floor: the deviations of that float32 run, in the measures of `ppo_ref.deviations`, are what `ppo_ref.FLOOR_STEP` and
    `FLOOR_CHAIN` record (worst over the cases and over two machines, rounded up to two digits); a larger figure fails
    here. torch runs on one thread while it is measured, so the figure does not depend on the machine's core count.
Sensitivity: the float32 oracle with one block of its gradient scaled (value tower x 1.2, first policy layer x 1.1, action
head x 1.1, log_std x 1.3 -- each passes `test_ppo_epochs_match_oracle`'s parameter comparison on these shapes) and with a
short last minibatch averaged over `batch_size` rows is out of tolerance at least tenfold in the measures the GPU tests use.

Columns: the five vector / state measures, the worst of the seven statistics columns, the ratio margin and the gradient norm
(chains: the smallest of the three steps). `python -m tests.test_ppo_ref` prints the tables.

Single steps (the row of `max_grad_norm` = 0.5; the worst line takes both runs):
    case                               grad      exp_avg   exp_avg_sq params    norm      statistic ratio     grad_norm
    4x2b_h32_norm_T2n1_bs2             4.3e-07   2.9e-07   5.0e-07   1.9e-08   3.0e-08   1.3e-05   1.4e-01   2.87    
    4x2b_h32_plain_T3n21_bs63          4.7e-07   4.9e-07   8.6e-07   1.9e-08   0.0e+00   5.1e-06   4.9e-03   1.93    
    4x2b_h32_norm_T4n16_bs64           5.4e-07   5.2e-07   7.8e-07   1.9e-08   1.5e-08   6.5e-07   2.9e-03   1.52    
    4x2b_h32_plain_T5n13_bs65          3.7e-07   2.8e-07   5.1e-07   1.9e-08   0.0e+00   2.1e-06   1.6e-03   1.65    
    4x2b_h32_norm_T2n65_bs130          6.2e-07   5.9e-07   7.5e-07   2.6e-08   4.4e-08   1.7e-06   7.1e-03   1.19    
    4x2b_h64_plain_T2n1_bs2            3.7e-07   3.3e-07   5.8e-07   1.9e-08   0.0e+00   6.2e-05   1.7e-01   3.17    
    4x2b_h64_norm_T3n21_bs63           3.5e-07   3.3e-07   5.2e-07   3.0e-08   3.6e-08   3.8e-06   1.1e-02   2.17    
    4x2b_h64_plain_T4n16_bs64          1.0e-06   9.5e-07   1.9e-06   1.9e-08   0.0e+00   1.2e-06   1.3e-02   2.03    
    4x2b_h64_norm_T5n13_bs65           7.4e-07   7.6e-07   1.5e-06   1.9e-08   4.6e-08   1.5e-06   2.2e-02   2       
    4x2b_h64_plain_T2n65_bs130         7.8e-07   9.2e-07   1.8e-06   2.4e-08   0.0e+00   2.1e-06   1.6e-03   1.72    
    4x2d_h32_plain_T2n1_bs2            6.0e-07   6.1e-07   7.7e-07   2.0e-08   0.0e+00   1.9e-06   1.2e-01   3.1     
    4x2d_h32_norm_T3n21_bs63           3.6e-07   3.5e-07   5.6e-07   3.6e-08   4.6e-08   8.0e-07   9.1e-03   0.901   
    4x2d_h32_plain_T4n16_bs64          4.4e-07   4.4e-07   6.8e-07   1.9e-08   0.0e+00   3.0e-06   5.9e-03   0.978   
    4x2d_h32_norm_T5n13_bs65           5.3e-07   5.5e-07   5.8e-07   1.9e-08   3.4e-08   4.4e-06   2.8e-03   0.635   
    4x2d_h32_plain_T2n65_bs130         5.0e-07   4.7e-07   6.5e-07   2.2e-08   0.0e+00   4.2e-06   1.5e-03   0.78    
    4x2d_h64_norm_T2n1_bs2             3.3e-07   2.8e-07   5.9e-07   1.9e-08   2.6e-08   2.3e-06   1.2e-01   4.38    
    4x2d_h64_plain_T3n21_bs63          3.6e-07   4.3e-07   8.3e-07   2.0e-08   0.0e+00   1.1e-06   1.1e-02   1.6     
    4x2d_h64_norm_T4n16_bs64           4.4e-07   4.4e-07   7.1e-07   1.9e-08   3.4e-08   2.7e-06   1.1e-02   1.52    
    4x2d_h64_plain_T5n13_bs65          5.0e-07   4.8e-07   6.4e-07   1.9e-08   0.0e+00   1.5e-06   1.3e-03   1.51    
    4x2d_h64_norm_T2n65_bs130          5.4e-07   5.0e-07   9.3e-07   1.9e-08   3.0e-08   1.1e-06   2.7e-03   0.77    
    17x6b_h32_norm_T2n1_bs2            4.6e-07   3.6e-07   7.1e-07   2.0e-08   5.0e-08   1.1e-05   7.3e-02   15.8    
    17x6b_h32_plain_T3n21_bs63         9.1e-07   9.3e-07   8.9e-07   2.0e-08   0.0e+00   2.5e-06   5.1e-03   2.21    
    17x6b_h32_norm_T4n16_bs64          1.1e-06   1.1e-06   1.0e-06   2.0e-08   5.7e-08   5.4e-06   4.6e-03   2.42    
    17x6b_h32_plain_T5n13_bs65         1.1e-06   9.8e-07   1.1e-06   1.9e-08   0.0e+00   6.5e-06   1.1e-02   2.26    
    17x6b_h32_norm_T2n65_bs130         6.5e-07   7.1e-07   1.2e-06   2.3e-08   5.6e-08   3.7e-06   1.6e-03   1.79    
    17x6b_h64_plain_T2n1_bs2           3.8e-07   4.2e-07   6.8e-07   1.9e-08   0.0e+00   2.5e-06   7.2e-02   21.5    
    17x6b_h64_norm_T3n21_bs63          2.9e-06   2.6e-06   4.2e-06   7.0e-08   4.8e-08   1.9e-05   8.2e-03   3.33    
    17x6b_h64_plain_T4n16_bs64         1.3e-06   1.2e-06   1.4e-06   8.3e-08   0.0e+00   8.1e-06   2.8e-03   3.32    
    17x6b_h64_norm_T5n13_bs65          1.9e-06   1.9e-06   1.7e-06   6.0e-08   4.9e-08   9.1e-05   1.1e-03   2.86    
    17x6b_h64_plain_T2n65_bs130        1.3e-06   1.2e-06   1.2e-06   6.0e-08   0.0e+00   6.3e-06   3.2e-03   2.17    
    27x8b_h32_plain_T2n1_bs2           1.1e-06   6.5e-07   1.2e-06   1.9e-08   0.0e+00   7.2e-06   3.3e-02   8.99    
    27x8b_h32_norm_T3n21_bs63          9.7e-07   9.7e-07   2.1e-06   1.3e-07   4.9e-08   7.9e-05   8.0e-03   2.21    
    27x8b_h32_plain_T4n16_bs64         1.0e-06   1.2e-06   1.7e-06   6.5e-08   0.0e+00   6.5e-06   1.2e-02   2.21    
    27x8b_h32_norm_T5n13_bs65          1.5e-06   1.5e-06   3.0e-06   3.1e-08   7.0e-08   4.7e-06   3.0e-03   2.17    
    27x8b_h32_plain_T2n65_bs130        9.8e-07   1.1e-06   1.5e-06   3.4e-08   0.0e+00   5.4e-05   3.2e-03   1.85    
    27x8b_h64_norm_T2n1_bs2            5.5e-07   5.3e-07   6.4e-07   6.8e-08   6.0e-08   5.5e-06   3.5e-02   11.6    
    27x8b_h64_plain_T3n21_bs63         1.2e-06   1.2e-06   1.6e-06   9.6e-08   0.0e+00   1.4e-05   1.2e-02   3.98    
    27x8b_h64_norm_T4n16_bs64          2.0e-06   2.0e-06   2.0e-06   4.3e-07   4.9e-08   3.4e-05   2.3e-03   3.69    
    27x8b_h64_plain_T5n13_bs65         1.2e-06   9.2e-07   1.9e-06   9.0e-08   0.0e+00   3.5e-06   2.1e-02   3.35    
    27x8b_h64_norm_T2n65_bs130         1.7e-06   1.5e-06   2.2e-06   1.2e-07   5.0e-08   8.2e-06   3.2e-03   2.44    
    33x1b_h32_norm_T2n1_bs2            3.9e-07   4.7e-07   7.9e-07   1.9e-08   6.0e-08   2.7e-06   1.2e-01   3.39    
    33x1b_h32_plain_T3n21_bs63         4.5e-07   4.4e-07   8.3e-07   1.9e-08   0.0e+00   1.6e-06   2.1e-02   1.62    
    33x1b_h32_norm_T4n16_bs64          6.2e-07   7.0e-07   1.5e-06   2.8e-08   7.8e-08   2.0e-06   1.2e-02   1.49    
    33x1b_h32_plain_T5n13_bs65         1.3e-06   1.2e-06   2.4e-06   1.9e-08   0.0e+00   1.6e-06   1.1e-02   1.4     
    33x1b_h32_norm_T2n65_bs130         4.2e-07   5.2e-07   1.0e-06   1.9e-08   4.5e-08   5.0e-07   8.8e-03   1.22    
    33x1b_h64_plain_T2n1_bs2           1.3e-06   1.3e-06   2.7e-06   2.8e-08   0.0e+00   4.0e-06   1.0e-01   7.65    
    33x1b_h64_norm_T3n21_bs63          7.2e-07   7.4e-07   1.5e-06   2.3e-08   5.0e-08   1.3e-06   2.5e-02   2.26    
    33x1b_h64_plain_T4n16_bs64         1.2e-06   1.4e-06   2.7e-06   1.9e-08   0.0e+00   2.0e-06   1.3e-03   2.08    
    33x1b_h64_norm_T5n13_bs65          4.4e-07   4.4e-07   8.0e-07   6.6e-08   5.2e-08   8.1e-07   3.8e-03   1.8     
    33x1b_h64_plain_T2n65_bs130        8.5e-07   7.6e-07   1.6e-06   3.1e-08   0.0e+00   2.3e-06   7.6e-03   1.61    
    64x16b_h32_plain_T2n1_bs2          1.4e-06   1.4e-06   1.2e-06   2.6e-07   0.0e+00   1.5e-05   3.4e-02   12.8    
    64x16b_h32_norm_T3n21_bs63         1.5e-06   1.5e-06   1.9e-06   7.7e-08   7.9e-08   8.3e-05   1.9e-03   3.29    
    64x16b_h32_plain_T4n16_bs64        2.8e-06   2.5e-06   4.0e-06   7.2e-08   0.0e+00   1.6e-04   7.0e-03   3.52    
    64x16b_h32_norm_T5n13_bs65         2.1e-06   2.1e-06   4.0e-06   5.9e-07   6.0e-08   9.0e-06   2.7e-03   3.4     
    64x16b_h32_plain_T2n65_bs130       1.5e-06   1.3e-06   1.6e-06   2.1e-07   0.0e+00   3.0e-05   5.3e-03   2.5     
    64x16b_h64_norm_T2n1_bs2           8.1e-07   6.9e-07   1.2e-06   4.3e-08   8.6e-08   1.0e-05   3.0e-02   17.4    
    64x16b_h64_plain_T3n21_bs63        2.1e-06   2.2e-06   3.8e-06   5.8e-07   0.0e+00   2.6e-06   3.7e-03   5.49    
    64x16b_h64_norm_T4n16_bs64         1.7e-06   1.7e-06   2.2e-06   1.5e-07   6.4e-08   4.4e-04   2.9e-03   5.65    
    64x16b_h64_plain_T5n13_bs65        2.4e-06   2.4e-06   2.8e-06   1.1e-07   0.0e+00   5.2e-06   7.3e-03   5.47    
    64x16b_h64_norm_T2n65_bs130        2.9e-06   2.8e-06   5.3e-06   1.5e-07   5.7e-08   3.3e-06   2.2e-03   3.85    
    20x13d_h32_norm_T2n1_bs2           3.7e-07   3.1e-07   5.6e-07   1.9e-08   8.2e-08   5.3e-04   1.9e-01   5.24    
    20x13d_h32_plain_T3n21_bs63        3.7e-07   3.2e-07   5.8e-07   3.9e-08   0.0e+00   4.8e-07   3.8e-03   1.39    
    20x13d_h32_norm_T4n16_bs64         3.3e-07   3.6e-07   4.6e-07   3.6e-08   4.4e-08   8.3e-08   6.4e-03   1.33    
    20x13d_h32_plain_T5n13_bs65        3.2e-07   3.3e-07   5.4e-07   1.9e-08   0.0e+00   7.3e-07   5.2e-03   0.984   
    20x13d_h32_norm_T2n65_bs130        5.5e-07   5.8e-07   9.5e-07   4.8e-08   6.8e-08   3.7e-07   1.1e-03   0.855   
    20x13d_h64_plain_T2n1_bs2          2.6e-07   2.6e-07   4.0e-07   2.0e-08   0.0e+00   1.5e-06   6.4e-02   10.1    
    20x13d_h64_norm_T3n21_bs63         4.1e-07   4.8e-07   8.6e-07   3.7e-08   6.0e-08   8.3e-06   4.9e-03   2.2     
    20x13d_h64_plain_T4n16_bs64        3.9e-07   4.2e-07   7.0e-07   2.1e-08   0.0e+00   5.6e-06   8.9e-03   2.44    
    20x13d_h64_norm_T5n13_bs65         4.2e-07   4.5e-07   8.1e-07   2.3e-08   6.7e-08   2.8e-06   2.4e-03   2.72    
    20x13d_h64_plain_T2n65_bs130       5.9e-07   5.5e-07   1.1e-06   5.6e-08   0.0e+00   1.1e-06   1.9e-03   1.69    
    17x6b_h32_norm_T1n1_bs1_rawadv     4.2e-07   4.5e-07   8.5e-07   1.9e-08   6.3e-08   4.1e-06   8.1e-03   25.1    
    4x2d_h64_norm_T1n1_bs1_rawadv      1.9e-07   2.3e-07   3.1e-07   1.9e-08   6.2e-08   1.7e-05   1.4e-01   5.39    
    17x6b_h32_norm_T4n3_bs12           7.4e-07   7.4e-07   1.6e-06   2.9e-08   6.3e-08   3.0e-06   8.4e-02   5.39    
    17x6b_h32_norm_T4n4_bs16           9.4e-07   1.1e-06   2.2e-06   3.8e-08   5.5e-08   2.9e-06   4.4e-03   4.01    
    17x6b_h32_norm_T4n35_bs140         6.5e-07   6.2e-07   1.1e-06   3.7e-08   5.7e-08   1.6e-05   3.6e-03   1.8     
    17x6b_h32_norm_T4n64_bs256         7.8e-07   7.8e-07   1.1e-06   4.3e-08   5.9e-08   2.7e-06   4.8e-03   1.65    
    17x6b_h32_norm_T4n144_bs576        1.1e-06   9.5e-07   1.9e-06   2.0e-08   5.7e-08   1.4e-06   1.7e-03   1.26    
    27x8b_h32_norm_T4n16_bs64          1.6e-06   1.6e-06   3.1e-06   1.7e-07   4.7e-08   6.7e-06   2.1e-02   2.56    
    27x8b_h32_norm_T4n64_bs256         1.6e-06   1.6e-06   2.4e-06   2.1e-07   4.3e-08   1.5e-05   1.7e-03   1.36    
    33x1b_h32_plain_T4n35_bs140        6.8e-07   6.5e-07   1.3e-06   2.6e-08   0.0e+00   1.2e-06   3.7e-03   1.37    
    64x16b_h32_norm_T4n16_bs64         2.1e-06   1.9e-06   2.2e-06   1.2e-07   6.1e-08   2.0e-04   8.6e-03   3.38    
    20x13d_h32_norm_T4n32_bs128        6.9e-07   6.5e-07   1.4e-06   2.3e-08   6.9e-08   5.1e-06   7.6e-03   0.942   
    4x2d_h32_plain_T4n4_bs16           2.5e-07   2.8e-07   5.0e-07   1.9e-08   0.0e+00   1.4e-05   3.7e-02   2.02    
    17x6b_h64_norm_T4n32_bs128         1.4e-06   1.4e-06   2.8e-06   7.0e-08   7.1e-08   4.6e-05   1.0e-03   2.22    
    27x8b_h64_norm_T4n50_bs200         1.5e-06   1.5e-06   1.7e-06   5.2e-08   5.8e-08   4.4e-05   1.7e-03   2.25    
    33x1b_h64_plain_T4n32_bs128        4.2e-07   4.2e-07   7.1e-07   1.9e-08   0.0e+00   1.5e-05   6.3e-03   2.08    
    worst, every quantity: grad 2.89e-06, exp_avg 2.89e-06, exp_avg_sq 5.54e-06, params 1.97e-06, norm 8.65e-08, pg_loss 4.42e-04, value_loss 2.97e-07, entropy_loss 1.92e-07, approx_kl 5.31e-04, loss 8.32e-05, grad_norm 5.32e-07, clip_coef 5.10e-07

Chains of three steps:
    case                               grad      exp_avg   exp_avg_sq params    norm      statistic ratio     grad_norm
    17x6b_h32_norm_T4n138_bs256        1.6e-06   7.0e-07   7.7e-07   5.6e-08   1.4e-07   1.3e-06   1.2e-03   1.4     
    20x13d_h32_norm_T4n56_bs96         4.1e-07   3.7e-07   7.0e-07   5.3e-08   9.4e-08   1.2e-06   5.3e-03   0.972   
    4x2d_h64_norm_T3n102_bs128         7.3e-07   3.4e-07   5.3e-07   4.3e-08   1.2e-07   1.7e-06   2.1e-03   1.08    
    worst, every quantity: grad 1.65e-06, exp_avg 7.03e-07, exp_avg_sq 7.68e-07, params 5.56e-08, norm 1.36e-07, pg_loss 1.66e-06, value_loss 4.39e-08, entropy_loss 4.47e-08, approx_kl 5.81e-07, loss 1.99e-07, grad_norm 2.20e-07, clip_coef 1.51e-07

    a second machine, worst lines only -- under pytest, then as `python -m tests.test_ppo_ref` prints them there:
    single steps: grad 6.60e-06, exp_avg 6.93e-06, exp_avg_sq 6.14e-06, params 2.08e-06, norm 8.65e-08, pg_loss 2.85e-04, value_loss 5.94e-07, entropy_loss 1.92e-07, approx_kl 4.82e-04, loss 9.65e-05, grad_norm 1.03e-06, clip_coef 1.03e-06
                  grad 5.40e-06, exp_avg 5.42e-06, exp_avg_sq 5.14e-06, params 1.51e-06, norm 8.65e-08, pg_loss 2.41e-04, value_loss 5.94e-07, entropy_loss 1.92e-07, approx_kl 4.82e-04, loss 9.65e-05, grad_norm 6.48e-07, clip_coef 6.70e-07
    chains:       grad 2.64e-06, exp_avg 6.86e-07, exp_avg_sq 1.09e-06, params 5.57e-08, norm 1.36e-07, pg_loss 2.53e-05, value_loss 1.14e-07, entropy_loss 2.08e-08, approx_kl 4.09e-07, loss 1.03e-07, grad_norm 1.32e-07, clip_coef 1.20e-07 (both ways)

    ppo_ref.FLOOR_STEP / FLOOR_CHAIN: per quantity the largest of these worst lines, rounded up to two digits
    (torch's float32 CPU kernels are chosen by processor: on one thread the figures still move by up to a factor of 2
    from host to host, which is what the factor 8 of TOL is for). A chain's loss statistics are compared per step on the
    device but only as the epoch's logged means here, so FLOOR_CHAIN takes the single-step floor for those five columns.
    ppo_ref.TOL_STEP: grad, exp_avg, exp_avg_sq 2e-5 (the ceiling: 8 x floor is 5e-5), params 1.7e-5, norm 7.0e-7,
    pg_loss 2e-3 (ceiling), value_loss 4.8e-6, entropy_loss 1.6e-6, approx_kl 4.3e-3, loss 7.8e-4, grad_norm 8.8e-6,
    clip_coef 8.8e-6. The relative measure of pg_loss, approx_kl and loss is weak where the statistic is a nearly cancelled
    sum (pg_loss = -mean(A min(r, clip r)) with normalised advantages; approx_kl of a single row).
"""
import contextlib

import numpy as np
import pytest
import torch as th

from tests import ppo_ref as R

SINGLE = [n for n, c in R.CASES.items() if c.steps == 1]
CHAINS = [n for n, c in R.CASES.items() if c.steps > 1]
assert sorted(CHAINS) == sorted(R.CHAIN_CASES) and all(R.CASES[n].steps == 3 for n in CHAINS)


@contextlib.contextmanager
def one_thread():
    """float32 sums on one thread: the measured floor does not depend on how many cores the machine has."""
    n = th.get_num_threads()
    th.set_num_threads(1)
    try:
        yield
    finally:
        th.set_num_threads(n)


def _logged_stats(o: R.OracleRun, max_grad_norm: float) -> np.ndarray:
    """The oracle's record in STAT_NAMES order: the epoch's logged means (`loss`: the last step's), the first step's norm,
    and the coefficient `clip_grad_norm_` forms from it in float32."""
    lg = o.logged
    norm = np.float32(o.norms[0])
    coef = min(np.float32(max_grad_norm) / (norm + np.float32(1e-6)), np.float32(1.0))
    return np.array([lg["train/policy_gradient_loss"], lg["train/value_loss"], lg["train/entropy_loss"], lg["train/approx_kl"],
                     lg["train/clip_fraction"], lg["train/loss"], norm, coef], np.float64)


def measure_single(case: R.Case, max_grad_norm: float):
    """(deviations of the float32 oracle from the reference step, the reference step)."""
    pol, host = R.build(case)
    ref = R.Reference(case, pol, host, max_grad_norm)
    step = ref.step_from(ref.initial)
    with one_thread():
        o = R.run_oracle(case, pol, host, max_grad_norm)
    assert len(o.grads) == 1
    stats = _logged_stats(o, max_grad_norm)
    assert R.clipped_rows(stats[4], step.rows) == R.clipped_rows(step.stats[4], step.rows), "clip_fraction is exact"
    assert o.nc == step.state.nc
    dev = R.deviations(dict(grad=o.grads[0], exp_avg=o.m, exp_avg_sq=o.v, params=o.P, stats=stats, nm=o.nm, nv=o.nv), step,
                       ref.sizes)
    return dev, step


def measure_chain(case: R.Case):
    pol, host = R.build(case)
    ref = R.Reference(case, pol, host, R.CLIPPED)
    steps = ref.chain(ref.initial, case.steps)
    with one_thread():
        o = R.run_oracle(case, pol, host, R.CLIPPED)
    assert len(o.grads) == case.steps
    last = steps[-1]
    # what the oracle logs of an epoch: means over its steps; `loss` is the last step's
    mean = np.mean([s.stats for s in steps], axis=0)
    mean[5] = last.stats[5]
    lg = _logged_stats(o, R.CLIPPED)
    assert abs(lg[4] - mean[4]) < 1e-7, "clip_fraction: the mean of three exact fractions, each rounded to float32"
    assert o.nc == last.state.nc
    dev = R.deviations(dict(exp_avg=o.m, exp_avg_sq=o.v, params=o.P, nm=o.nm, nv=o.nv), last, ref.sizes)
    for j, name in enumerate(R.STAT_NAMES[:6]):
        if name != "clip_fraction":
            dev[name] = abs(lg[j] - mean[j]) / abs(mean[j])
    dev["grad"] = max(max(R.block_deviation(g, s.grad, ref.sizes)) for g, s in zip(o.grads, steps))
    dev["grad_norm"] = max(abs(float(np.float32(n)) - s.total_norm) / s.total_norm for n, s in zip(o.norms, steps))
    coefs = [min(np.float32(R.CLIPPED) / (np.float32(n) + np.float32(1e-6)), np.float32(1.0)) for n in o.norms]
    dev["clip_coef"] = max(abs(float(c) - s.clip_coef) / s.clip_coef for c, s in zip(coefs, steps))
    return dev, steps


def _row(name, dev, margin, norm):
    cols = ("grad", "exp_avg", "exp_avg_sq", "params", "norm")
    stat = max(dev[q] for q in R.MEASURED_STATS)
    return (f"    {name:<34s} " + " ".join(f"{dev.get(q, 0.0):<9.1e}" for q in cols) + f" {stat:<9.1e} {margin:<9.1e} {norm:<8.3g}")


def _assert_under_the_floor(dev, floor):
    print("    " + " ".join(f"{q}={v:.4g}" for q, v in dev.items()))
    over = {q: (float(f"{v:.4g}"), floor[q]) for q, v in dev.items() if v > floor[q]}
    assert not over, f"float32 deviates by more than the recorded floor (measured, recorded): {over}"


@pytest.mark.parametrize("name", SINGLE)
def test_single_step_matches_the_float32_oracle_and_meets_the_guards(name):
    case = R.CASES[name]
    for max_norm in (R.UNCLIPPED, R.CLIPPED):
        dev, step = measure_single(case, max_norm)
        print("\n" + _row(name, dev, step.ratio_margin, step.total_norm))
        R.assert_guards([step], max_norm == R.CLIPPED, max_norm, name)
        assert (step.clip_coef == 1.0) == (max_norm == R.UNCLIPPED)
        _assert_under_the_floor(dev, R.FLOOR_STEP)


@pytest.mark.parametrize("name", CHAINS)
def test_chain_matches_the_float32_oracle_and_meets_the_guards(name):
    case = R.CASES[name]
    dev, steps = measure_chain(case)
    print("\n" + _row(name, dev, min(s.ratio_margin for s in steps), min(s.total_norm for s in steps)))
    R.assert_guards(steps, True, R.CLIPPED, name)
    assert [s.rows for s in steps] == [case.bs, case.bs, case.rows - 2 * case.bs] and steps[-1].rows < case.bs
    _assert_under_the_floor(dev, R.FLOOR_CHAIN)


def test_every_gpu_case_is_a_reference_case():
    listed = set(R.GRAD_CASES + R.STEP32_CASES + R.STEP64_CASES + R.CHAIN_CASES)
    assert listed == set(R.CASES)


def test_the_barrier_epoch_forms_fit_only_their_own_shapes():
    """`plan_epoch`'s chunk conditions, restated: the 64-, 128- and 200-row shapes select neither barrier form (modes 2 and
    3 run them on two launches per minibatch), the shapes of STEP64_BARRIER_CASES select both."""
    assert [R.param_count(4, 2, 64, True), R.param_count(17, 6, 64, False), R.param_count(27, 8, 64, False)] == [9155, 11085, 12497]
    for n in R.STEP64_MODE_CASES:
        assert R.barrier_forms_fit(R.CASES[n]) == (False, False), n
    for n in R.STEP64_BARRIER_CASES:
        assert R.barrier_forms_fit(R.CASES[n]) == (True, True), n


def test_tolerances_follow_from_the_floor_and_stay_under_the_ceilings():
    for floor, ceiling, tol in ((R.FLOOR_STEP, R.CEILING_STEP, R.TOL_STEP), (R.FLOOR_CHAIN, R.CEILING_CHAIN, R.TOL_CHAIN)):
        assert set(floor) == set(ceiling) == set(tol) == set(R.QUANTITIES)
        for q in tol:
            assert floor[q] > 0.0, f"{q}: no measured floor recorded"
            derived = min(ceiling[q], max(8.0 * floor[q], 4.0 * R.ULP))
            assert tol[q] == (ceiling[q] if q in R.EXPLAINED else derived) <= ceiling[q]
    assert R.CEILING_STEP["params"] == 2e-5 and R.CEILING_CHAIN["params"] == 4e-5


def test_float64_adam_is_torch_adam():
    """`Reference.step_from`'s and `clip_and_adam`'s optimiser step against `torch.optim.Adam` and `clip_grad_norm_` in
    float64, over three steps."""
    case = R.CASES[R.CHAIN_CASES[0]]
    pol, host = R.build(case)
    ref = R.Reference(case, pol, host, R.CLIPPED)
    steps = ref.chain(ref.initial, 3)
    p = th.nn.Parameter(ref.initial.P.clone())
    opt = th.optim.Adam([p], lr=R.LR, betas=(R.BETA1, R.BETA2), eps=R.ADAM_EPS)
    state = ref.initial
    for s in steps:
        p.grad = s.grad.clone()
        norm = th.nn.utils.clip_grad_norm_([p], R.CLIPPED)
        opt.step()
        assert abs(float(norm) - s.total_norm) <= 1e-13 * s.total_norm
        th.testing.assert_close(s.state.P, p.detach(), rtol=1e-13, atol=1e-15)
        th.testing.assert_close(s.state.m, opt.state[p]["exp_avg"], rtol=1e-12, atol=0)
        th.testing.assert_close(s.state.v, opt.state[p]["exp_avg_sq"], rtol=1e-12, atol=0)
        total_norm, coef, m, v, P = R.clip_and_adam(s.grad, state, R.CLIPPED)
        assert total_norm == s.total_norm and coef == s.clip_coef
        assert th.equal(m, s.state.m) and th.equal(v, s.state.v) and th.equal(P, s.state.P)
        state = s.state


# ---- sensitivity: what `test_ppo_epochs_match_oracle` lets through is caught here -----------------------------------------------
def _scale(names, factor):
    def tamper(step, pol, rows):
        for n, p in pol.named_parameters():
            if any(n.startswith(prefix) for prefix in names):
                p.grad.mul_(factor)
    return tamper


INJECTED = {
    "value tower x 1.2": (_scale(("mlp_extractor.value_net", "value_net"), 1.2), False),
    "policy layer 1 x 1.1": (_scale(("mlp_extractor.policy_net.0",), 1.1), False),
    "action head x 1.1": (_scale(("action_net",), 1.1), True),
    "log_std x 1.3": (_scale(("log_std",), 1.3), True),
}


@pytest.mark.parametrize("shape,what", [(s, w) for s in R.SENSITIVITY_SHAPES for w in INJECTED
                                        if not (s[3] and w.startswith("log_std"))],   # (a Categorical head has no log_std)
                         ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_a_scaled_gradient_block_exceeds_the_tolerance_tenfold(shape, what):
    """The float32 oracle with one block of its first step's gradient scaled, against the reference step, in the measures and
    tolerances the GPU tests use: the gradient and exp_avg (one step, no clipping: exp_avg = (1 - beta1) g) must be out by
    at least 10 x TOL; a scaled head or log_std must show in grad_norm as well."""
    case = R.sensitivity_case(*shape)
    tamper, in_norm = INJECTED[what]
    pol, host = R.build(case)
    ref = R.Reference(case, pol, host, R.UNCLIPPED)
    step = ref.step_from(ref.initial)
    # (2 048 rows: among the first 1 500 seeds none keeps every ratio 1e-3 away from the clip bounds -- the best reaches
    #  9.2e-4. That guard protects the exact comparison of clip_fraction, which this test does not make; float32 moves a
    #  ratio by 1e-6, far less than the 4e-5 this seed leaves. The margin stays what it is; the other guards are asserted.)
    R.assert_guards([step], False, R.UNCLIPPED, case.name, ratio=case.bs < 2048)
    with one_thread():
        clean = R.run_oracle(case, R.build(case)[0], host, R.UNCLIPPED)
        bad = R.run_oracle(case, pol, host, R.UNCLIPPED, tamper=lambda k, p, rows: tamper(k, p, rows) if k == 0 else None)
    sizes = ref.sizes
    m1 = lambda o: (1.0 - R.BETA1) * o.grads[0].double()     # exp_avg after step 1, as the forms without a gradient show it
    base = R.deviations(dict(grad=clean.grads[0], exp_avg=m1(clean)), step, sizes)
    dev = R.deviations(dict(grad=bad.grads[0], exp_avg=m1(bad)), step, sizes)
    norm_dev = abs(bad.norms[0] - step.total_norm) / step.total_norm
    print(f"\n    {case.name} {what}: grad {dev['grad']:.2e} (clean {base['grad']:.1e}, tol {R.TOL_STEP['grad']:.1e}), "
          f"grad_norm {norm_dev:.2e} (tol {R.TOL_STEP['grad_norm']:.1e})")
    assert base["grad"] <= R.TOL_STEP["grad"] and base["exp_avg"] <= R.TOL_STEP["exp_avg"]
    assert dev["grad"] >= 10.0 * R.TOL_STEP["grad"] and dev["exp_avg"] >= 10.0 * R.TOL_STEP["exp_avg"]
    if in_norm:
        assert norm_dev >= 10.0 * R.TOL_STEP["grad_norm"]


@pytest.mark.parametrize("name", [R.CHAIN_CASES[0], R.CHAIN_CASES[1]])
def test_a_short_last_minibatch_averaged_over_the_full_size_exceeds_the_tolerance_tenfold(name):
    """The last minibatch's gradient divided by `batch_size` instead of its own row count (x rows / batch_size on every
    element): the last step's gradient and the final exp_avg against the reference chain."""
    case = R.CASES[name]
    pol, host = R.build(case)
    ref = R.Reference(case, pol, host, R.UNCLIPPED)
    steps = ref.chain(ref.initial, case.steps)

    def tamper(k, p, rows):
        if rows < case.bs:
            for q in p.parameters():
                q.grad.mul_(rows / case.bs)
    with one_thread():
        bad = R.run_oracle(case, pol, host, R.UNCLIPPED, tamper=tamper)
    dev = R.deviations(dict(grad=bad.grads[-1], exp_avg=bad.m), steps[-1], ref.sizes)
    print(f"\n    {name}: last gradient {dev['grad']:.2e}, exp_avg {dev['exp_avg']:.2e} (tol {R.TOL_CHAIN['grad']:.1e})")
    assert dev["grad"] >= 10.0 * R.TOL_CHAIN["grad"] and dev["exp_avg"] >= 10.0 * R.TOL_CHAIN["exp_avg"]


# ---- `python -m tests.test_ppo_ref`: the seed search and the tables of this docstring ----------------------------------------------
def _find_seed(case: R.Case, chain: bool, limit: int = 4000):
    import dataclasses
    for seed in range(limit):
        c = dataclasses.replace(case, seed=seed)
        pol, host = R.build(c)
        try:
            for max_norm in ((R.CLIPPED,) if chain else (R.UNCLIPPED, R.CLIPPED)):
                ref = R.Reference(c, pol, host, max_norm)
                steps = ref.chain(ref.initial, c.steps) if chain else [ref.step_from(ref.initial)]
                R.assert_guards(steps, max_norm == R.CLIPPED, max_norm)
        except AssertionError:
            continue
        return seed
    raise RuntimeError(case.name)


if __name__ == "__main__":
    import sys
    if "seeds" in sys.argv:
        found = {}
        for c in list(R.CASES.values()) + [R.sensitivity_case(*s) for s in R.SENSITIVITY_SHAPES]:
            try:
                s = _find_seed(c, c.steps > 1 and not c.name.startswith("sens_"), 1500 if c.name.startswith("sens_") else 4000)
            except RuntimeError:
                print(c.name, "none")
                continue
            if s:
                found[c.name] = s
            print(c.name, s, flush=True)
        print("SEEDS =", found)
    else:
        for group, names, fn in (("single steps", SINGLE, None), ("chains", CHAINS, measure_chain)):
            worst = dict.fromkeys(R.QUANTITIES, 0.0)
            print(group)
            for n in names:
                if fn is None:
                    for mx in (R.UNCLIPPED, R.CLIPPED):
                        dev, step = measure_single(R.CASES[n], mx)
                        worst = {q: max(worst[q], dev.get(q, 0.0)) for q in worst}
                    print(_row(n, dev, step.ratio_margin, step.total_norm))
                else:
                    dev, steps = fn(R.CASES[n])
                    worst = {q: max(worst[q], dev.get(q, 0.0)) for q in worst}
                    print(_row(n, dev, min(s.ratio_margin for s in steps), min(s.total_norm for s in steps)))
            print("    worst", {q: float(f"{v:.4g}") for q, v in worst.items()})
