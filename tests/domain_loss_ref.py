"""The baselines' weighted BCE + CORAL loss as a closed form in torch fp64 on the CPU: what
csrc/domain_loss_ops.hip computes (reference FusionModule.py:341-390, coral_loss/coral.py:5-37),
with both gradients written out rather than taken by autograd.

With x_i the pooled feature rows, c_i the domain codes (0 source / INTERNAL, 1 target / BTXRD,
anything else in neither), n_s, n_t the counts, mu_s, mu_t the domains' column means and
w_i = +1 / (n_s - 1), -1 / (n_t - 1) or 0:

    Delta = sum_i w_i x_i x_i^T - mu_s mu_s^T / (n_s - 1) + mu_t mu_t^T / (n_t - 1)
    coral = lambda ||Delta||_F^2 / (4 D^2)
    d coral / d x_i = (lambda w_i / D^2) (x_i - mu_dom(i) / n_dom(i)) Delta

(the reference's "covariance" subtracts the mean outer product once, not n times), both exactly 0
where n_s <= 1, n_t <= 1 or lambda == 0; and with u_i = w0 where y_i == 0, else w1:

    cls = (1 / N) sum_i u_i (max(z_i, 0) - z_i y_i + log1p(exp(-|z_i|)))
    d cls / d z_i = u_i (sigmoid(z_i) - y_i) / N
"""
import torch

CODES = {"INTERNAL": 0, "BTXRD": 1}


def codes_of(dataset):
    return torch.tensor([CODES.get(d, 2) for d in dataset], dtype=torch.uint8)


def domain_loss_ref(features, logits, labels, codes, w0, w1, coral_lambda):
    """{"total", "cls", "coral"} (0-dim fp64), "g_feat" (fp64, the shape of features) and
    "g_logits" (fp64 [N]).  features [N, D] or [N, D, h, w] (pooled by the spatial mean); the
    inputs are widened to fp64 as given, so fp32 inputs are evaluated exactly as stored."""
    x4 = features.detach().double().cpu()
    x = x4.mean((2, 3)) if x4.dim() == 4 else x4
    z = logits.detach().double().cpu().reshape(-1)
    yl = labels.detach().cpu().reshape(-1)
    y = yl.double()
    codes = torch.as_tensor(codes).cpu().reshape(-1)
    N, D = x.shape
    w0, w1, lam = float(w0), float(w1), float(coral_lambda)
    u = torch.where(yl == 0, torch.tensor(w0, dtype=torch.float64), torch.tensor(w1, dtype=torch.float64))
    cls = (u * (z.clamp_min(0.0) - z * y + torch.log1p(torch.exp(-z.abs())))).sum() / N
    g_logits = u * (torch.sigmoid(z) - y) / N
    src, tgt = codes == 0, codes == 1
    ns, nt = int(src.sum()), int(tgt.sum())
    coral = torch.zeros((), dtype=torch.float64)
    g = torch.zeros_like(x)
    if ns > 1 and nt > 1 and lam != 0.0:
        w = torch.zeros(N, dtype=torch.float64)
        w[src], w[tgt] = 1.0 / (ns - 1), -1.0 / (nt - 1)
        mu_s, mu_t = x[src].mean(0), x[tgt].mean(0)
        delta = (x * w[:, None]).T @ x - torch.outer(mu_s, mu_s) / (ns - 1) + torch.outer(mu_t, mu_t) / (nt - 1)
        coral = lam * (delta * delta).sum() / (4.0 * D * D)
        shift = torch.zeros_like(x)
        shift[src], shift[tgt] = mu_s / ns, mu_t / nt
        g = (lam * w / (D * D))[:, None] * ((x - shift) @ delta)
        g[~(src | tgt)] = 0.0
    if x4.dim() == 4:
        g = (g / (x4.shape[2] * x4.shape[3]))[:, :, None, None].expand_as(x4).contiguous()
    return {"total": cls + coral, "cls": cls, "coral": coral, "g_feat": g, "g_logits": g_logits}
