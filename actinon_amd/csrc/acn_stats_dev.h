/* acn_stats_dev.h -- the rules of the statistics record { n, mean.xyz, m2.xyz, 0 } that every kernel which reads one applies
 * (k_lens.hip, k_denoise.hip, k_denoise_layers.hip; include/actinon_hip.h states them under ACN_STATS_STRIDE). */
#ifndef ACN_STATS_DEV_H
#define ACN_STATS_DEV_H

#include <hip/hip_runtime.h>

/* a record whose [ 0 ] is not a finite number >= 1 is EMPTY (a NaN fails both comparisons) */
__device__ static inline bool stats_empty( double n ) { return !( n >= 1.0 && n < __builtin_inf() ); }

/* the variance of the mean of one channel: m2 its sum of squared deviations over the n > 1 samples of a record */
__device__ static inline double stats_var_of_mean( double m2, double n ) { return ( m2 / ( n - 1.0 ) ) / n; }

#endif
