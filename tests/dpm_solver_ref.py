"""DPM-Solver++ (2M) (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models", Algorithm 2),
restated in float64 for the tests of scheduler="dpm++" -- python floats on the float32 alphas_cumprod, nothing from the package.

Notation.  a = alphas_cumprod[t], alpha = sqrt(a), sigma = sqrt(1 - a), lambda(a) = ln(alpha / sigma) = 1/2 ln(a / (1 - a)).
Leading spacing: r = T // K, t_i = (K - 1 - i) r; the step at position i goes from t_i to prev = t_i - r with
h_i = lambda(a_prev) - lambda(a_t).  D_i is the data prediction at position i (the clipped, in-painted network output).

  textbook (2M):  x_prev = (sigma_prev / sigma_t) x_t - alpha_prev (e^{-h_i} - 1) [(1 + 1 / (2 rho)) D_i - 1 / (2 rho) D_{i-1}],
                  rho = h_{i-1} / h_i                                                   (first order: the bracket is D_i)
  three terms:    x_prev = c0 D_i + c1 x_t + kappa_i (D_i - D_{i-1}),
                  c1 = sigma_prev / sigma_t,  c0 = alpha_prev - c1 alpha_t  (the DDIM row at eta = 0),
                  kappa_i = alpha_prev (1 - e^{-h_i}) h_i / (2 h_{i-1}).

kappa_i = 0 at position 0, for solver_order 1, at the terminal position K - 1 (prev < 0: the network output is the result) and, with
lower_order_final, at position K - 2 (the update that lands on timestep 0)."""
import math


def timesteps(T, K):
    r = T // K
    return [(K - 1 - i) * r for i in range(K)], r


def lam(a):
    return 0.5 * math.log(a / (1.0 - a))


def ddim_row(a_t, a_prev):
    c1 = math.sqrt(1.0 - a_prev) / math.sqrt(1.0 - a_t)
    return math.sqrt(a_prev) - c1 * math.sqrt(a_t), c1


def schedule(acp, T, K, solver_order=2, lower_order_final=True):
    """-> (timesteps, [(c0, c1)] * K, [kappa] * K) as python floats; acp: the T float32 alphas_cumprod of one beta schedule.
    The entries of the terminal position K - 1 are those of a_prev = 1 (c0 = 1, c1 = 0) and kappa = 0: the step does not use them."""
    ts, r = timesteps(T, K)
    a = [float(x) for x in acp]
    rows, kappa = [], []
    for i, t in enumerate(ts):
        prev = t - r
        if prev < 0:
            rows.append((1.0, 0.0))
            kappa.append(0.0)
            continue
        rows.append(ddim_row(a[t], a[prev]))
        second = solver_order == 2 and i >= 1 and not (lower_order_final and i == K - 2)
        if not second:
            kappa.append(0.0)
            continue
        h, h_last = lam(a[prev]) - lam(a[t]), lam(a[t]) - lam(a[ts[i - 1]])
        kappa.append(math.sqrt(a[prev]) * (1.0 - math.exp(-h)) * h / (2.0 * h_last))
    return ts, rows, kappa


def textbook_step(a_t, a_prev, a_last, x_t, d, d_last):
    """One 2M update in the textbook form (d_last / a_last None: the first-order update).  a_last: alphas_cumprod at the previous
    step's timestep.  Works on floats and on float64 tensors."""
    h = lam(a_prev) - lam(a_t)
    ratio = math.sqrt(1.0 - a_prev) / math.sqrt(1.0 - a_t)
    bracket = d
    if d_last is not None:
        rho = (lam(a_t) - lam(a_last)) / h
        bracket = (1.0 + 1.0 / (2.0 * rho)) * d - (1.0 / (2.0 * rho)) * d_last
    return ratio * x_t - math.sqrt(a_prev) * (math.exp(-h) - 1.0) * bracket


def three_term_step(row, kappa, x_t, d, d_last):
    """the form the kernels evaluate, in their order: c0 D + c1 x, then + kappa (D - D_last) only where kappa != 0"""
    out = row[0] * d + row[1] * x_t
    if kappa != 0.0:
        out = out + kappa * (d - d_last)
    return out


# ---- data with a known answer: x0 ~ N(mu, s^2) per element
def gaussian_denoiser(a, x, mu, s):
    """E[x0 | x_t = x] for x0 ~ N(mu, s^2) and x_t = sqrt(a) x0 + sqrt(1 - a) eps"""
    return mu + math.sqrt(a) * s * s / (a * s * s + 1.0 - a) * (x - math.sqrt(a) * mu)


def gaussian_flow(a_from, a_to, x, mu, s):
    """Exact transport of the probability-flow ODE from the marginal at a_from to the one at a_to: the marginals are
    N(sqrt(a) mu, a s^2 + 1 - a) and the (linear) flow keeps the standardised coordinate."""
    sd = lambda a: math.sqrt(a * s * s + 1.0 - a)
    return math.sqrt(a_to) * mu + sd(a_to) / sd(a_from) * (x - math.sqrt(a_from) * mu)
