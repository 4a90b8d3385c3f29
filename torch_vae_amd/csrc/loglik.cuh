// Importance-weighted log-likelihood and per-sample ELBO (vae_log_likelihood, vae_api.hip): the kernels around the decoder.
//   log w[k,b] = log p(x_b|z_kb) + log p(z_kb) - log q(z_kb|x_b),   z_kb = eps_kb * exp(0.5 lv_b) + mu_b
//   log p(x_b) ~ logsumexp_k log w[k,b] - log K        (Burda et al., IWAE)
//   elbo[b]    = mean_k log p(x_b|z_kb) - KL(q(z|x_b) || N(0, I))
// log p(x|z) comes from the per-sample mode of the output-conv kernels (one partial per tile, conv_mfma.cuh / edge_kernels.cuh);
// everything from there on is f64 and summed in a fixed order, so the result does not depend on how K is chunked.
#pragma once
#include "edge_kernels.cuh"

// z of the draws k0 .. k0+nk-1 for the whole batch and, per draw, log p(z) - log q(z|x) = sum_l (-z^2/2 + eps^2/2 + lv/2)
// (the 2 pi terms cancel).  eps[k,b,l] is element (k*B + b)*L + l of the caller's [K,B,L] array or of the counter generator's
// stream 6; z is formed as latent_fwd_kernel forms it (models.py:181-183).  One thread per draw (row r = (k - k0)*B + b).
struct IwLatentArgs {
    const float* mu; const float* lv;   // [B, L] of the encoder pass
    const float* eps;                   // [K, B, L] or null (counter generator)
    float* z;                           // [nk*B, L]: the decoder's input
    double* lat;                        // [nk*B]
    int B, L, k0, nk; unsigned long long seed;
};
static __global__ void iw_latent_kernel(IwLatentArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nk * a.B) return;
    const int b = r % a.B;
    const long g = (long)a.k0 * a.B + r;
    double acc = 0.0;
    for (int l = 0; l < a.L; ++l) {
        const long i = g * a.L + l;
        const float e = a.eps ? a.eps[i] : counter_normal_at((unsigned long long)i, a.seed, 6ULL);
        const float m = a.mu[b * a.L + l], v = a.lv[b * a.L + l];
        const float sd = expf(0.5f * v);
        const float zz = e * sd + m;
        a.z[(long)r * a.L + l] = zz;
        acc += -0.5 * (double)zz * (double)zz + 0.5 * (double)e * (double)e + 0.5 * (double)v;
    }
    a.lat[r] = acc;
}

// Combine, first half (after each chunk's decoder pass): per draw, the tile partials summed in tile order give
// s = sum over pixels of the reconstruction term; log p(x|z) = -s - cst (BCE: cst = 0; MSE: cst = H*W/2 * log(pi)), and
// log w = log p(x|z) + lat.  Row r of the chunk is draw (row0 + r) of the call.
static __global__ void loglik_rows_kernel(const double* __restrict__ part, int ntile, const double* __restrict__ lat, int nrows,
                                          long row0, double cst, double* __restrict__ lpx, double* __restrict__ lw) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const double* p = part + (long)r * ntile;
    double s = 0.0;
    for (int t = 0; t < ntile; ++t) s += p[t];
    const double v = -s - cst;
    lpx[row0 + r] = v;
    lw[row0 + r] = v + lat[r];
}

// Combine, second half (once per call): per sample b, max-shifted logsumexp over k of log w minus log K, and the ELBO with the
// analytic KL (summed over l, beta = 1).  One thread per sample; k in increasing order.
static __global__ void loglik_final_kernel(const double* __restrict__ lpx, const double* __restrict__ lw, const float* __restrict__ mu,
                                           const float* __restrict__ lv, int K, int B, int L, double* __restrict__ ll, double* __restrict__ elbo) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double mx = -INFINITY, sp = 0.0;
    for (int k = 0; k < K; ++k) { mx = fmax(mx, lw[(long)k * B + b]); sp += lpx[(long)k * B + b]; }
    double s = 0.0;
    if (isfinite(mx)) for (int k = 0; k < K; ++k) s += exp(lw[(long)k * B + b] - mx);
    ll[b] = (isfinite(mx) ? mx + log(s) : mx) - log((double)K);
    double kl = 0.0;
    for (int l = 0; l < L; ++l) {
        const double m = mu[b * L + l], v = lv[b * L + l];
        kl += 1.0 + v - m * m - exp(v);
    }
    elbo[b] = sp / (double)K + 0.5 * kl;
}
