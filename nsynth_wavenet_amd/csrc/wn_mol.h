// Discretised-logistic mixture (MoL) arithmetic shared by the teacher's scoring kernel (tg_log_prob_kernel,
// wn_teacher.hip) and the distillation cross entropy (wn_distill.hip): loss_func.mol_log_probs (wavenet/loss_func.py:22-63).
//
// The mass of the bin around x, cdf(x + 1/Q) - cdf(x - 1/Q), is formed as sigma(a) sigma(-b) (1 - e^-(a-b)) with
// a = inv_s (x - mean + 1/Q), b = inv_s (x - mean - 1/Q) and a - b = 2 inv_s / Q taken directly: the difference of two
// float32 sigmoids the reference's formula takes keeps about two digits of a mass of 1/65 536.  The factor 1 - e^-(a-b)
// depends on the component only (wn_mol_bin_factor), so a caller that evaluates one row at many x forms it once.
#pragma once
#include <hip/hip_runtime.h>

__device__ inline float wn_softplus(float v) { return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))); }
__device__ inline float wn_sigmoid(float v) {
    const float e = expf(-fabsf(v));
    return v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// edges of the outermost bins (loss_func.py:52-55): below min_thres the lower tail, above max_thres the upper tail
__device__ inline void wn_mol_thresholds(int Q, float& min_thres, float& max_thres) {
    max_thres = ((float)(Q - 1) - 0.5f) / ((float)Q * 0.5f) - 1.0f;
    min_thres = 0.5f / ((float)Q * 0.5f) - 1.0f;
}

// 1 - e^-(a-b) of one component: inv = exp(-max(log_scale, -7)), iq = 1/Q
__device__ inline float wn_mol_bin_factor(float inv, float iq) { return -expm1f(-2.0f * inv * iq); }

// log-probability of one component at x (before the mixture weight): log_cdf_plus / log_one_minus_cdf_min at the edges,
// log(max(mass, 1e-12)) inside (loss_func.py:56-60).  c = x - mean, d = wn_mol_bin_factor(inv, iq).
__device__ inline float wn_mol_component_lp(float x, float c, float inv, float iq, float d, float min_thres, float max_thres) {
    const float plus = inv * (c + iq), mn = inv * (c - iq);
    const float delta = wn_sigmoid(plus) * wn_sigmoid(-mn) * d;
    return x < min_thres ? plus - wn_softplus(plus) : (x > max_thres ? -wn_softplus(mn) : logf(fmaxf(delta, 1e-12f)));
}

// derivatives of wn_mol_component_lp at x in the same form (TensorFlow's tie conventions): dx = d lp / d x (= -d lp / d mean),
// dinv = d lp / d inv_s.  Inside: log sigma(a) + log sigma(-b) + log(1 - e^-(a-b)) with a - b = 2 inv_s / Q, zero below the
// 1e-12 floor; lower tail log sigma(a); upper tail log sigma(-b).
__device__ inline void wn_mol_component_grad(float x, float c, float inv, float iq, float d, float min_thres, float max_thres,
                                             float& dx, float& dinv) {
    const float plus = inv * (c + iq), mn = inv * (c - iq);
    float gp = 0.f, gm = 0.f, ge = 0.f;
    if (x < min_thres) {
        gp = wn_sigmoid(-plus);
    } else if (x > max_thres) {
        gm = -wn_sigmoid(mn);
    } else if (wn_sigmoid(plus) * wn_sigmoid(-mn) * d >= 1e-12f) {
        gp = wn_sigmoid(-plus);
        gm = -wn_sigmoid(mn);
        ge = 2.0f * iq / expm1f(2.0f * inv * iq);
    }
    dx = inv * (gp + gm);
    dinv = (c + iq) * gp + (c - iq) * gm + ge;
}
