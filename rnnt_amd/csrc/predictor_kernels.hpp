// predictor_kernels.hpp — the row kernels of predictor.hip that lstm.hip runs too: LayerNorm over the last
// dimension (forward with its per-row mean / rstd, backward with T = dy * xhat for the affine's column sums)
// and the embedding table's gradient.  `ids` non-NULL: row m of X is embedding row ids[m] (X = the table, S rows).
#pragma once
#include "common.hpp"

void launch_ln_fwd(const float *X, const int64_t *ids, int S, const float *gamma, const float *beta, float eps, int M, int N,
                   float *Y, float *stats, hipStream_t st);
void launch_ln_bwd(const float *X, const int64_t *ids, int S, const float *gamma, const float *stats, const float *dY, int M, int N,
                   float *dX, float *T, hipStream_t st);
// dEmb[s,:] = sum over the rows m (ascending) with ids[m] == s of dX0[m,:]; E <= 2048
void launch_embed_bwd(const int64_t *ids, const float *dX0, int M, int E, int S, float *dEmb, hipStream_t st);
