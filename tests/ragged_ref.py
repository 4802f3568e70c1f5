"""fp64 restatement of Inception1D on series of different lengths
(HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:474-515 applied to every series on its own
length; the per-sample windows of lib/Hodge_Dataset.py:131-133).

Everything per series is F.conv1d / F.max_pool1d / max / mean on that series
alone.  BatchNorm is the only batch-coupled step and is written out by
formula: in training mode the mean and the BIASED variance over all valid
(series, step) positions normalise, and running_var receives the UNBIASED one
with n = the number of valid positions; in eval mode the running statistics.

ragged_forward takes the module's state_dict as a dict of tensors (leaves that
may require grad) so the caller differentiates it with autograd.
"""
import torch
import torch.nn.functional as F

LENS_A = [40, 24, 1, 2, 37, 3, 21]   # sum 128: a series boundary on the tile edge at row 64
LENS_B = [39, 26, 1, 5, 40, 2, 30]   # sum 143: boundaries at rows 65 and 66, a partly dead tile
T_MAX = 40


def _bn(hs, sd, name, training, eps, stats):
    """hs: list of [1, C, len_s]; pooled statistics over every position."""
    w, b = sd[name + ".weight"], sd[name + ".bias"]
    if training:
        cat = torch.cat(hs, dim=2)[0]  # [C, sum len]
        n = cat.shape[1]
        mean = cat.mean(dim=1)
        var = ((cat - mean[:, None]) ** 2).mean(dim=1)
        stats[name] = (mean.detach(), (var * n / max(n - 1, 1)).detach(), n)
    else:
        mean, var = sd[name + ".running_mean"], sd[name + ".running_var"]
    return [(h - mean[None, :, None]) / torch.sqrt(var[None, :, None] + eps)
            * w[None, :, None] + b[None, :, None] for h in hs]


def _gap(v, dim):
    """Smallest difference between the two largest entries along dim."""
    if v.shape[dim] < 2:
        return float("inf")
    s = torch.sort(v, dim=dim, descending=True)[0]
    g = s.select(dim, 0) - s.select(dim, 1)
    g = g[torch.isfinite(g)]
    return float(g.min()) if g.numel() else float("inf")


def ragged_forward(sd, x, lens, m=3, slope=0.1, training=True, eps=1e-5, info=None):
    """out [S, 8 * num_channels] of x [S, >= max(lens)] (columns past lens[s]
    are never read).  info (a dict) receives 'margin', the smallest distance
    of any LeakyReLU input from 0 and of any max (pool window, readout) from
    its runner-up, and 'stats', {bn: (mean, unbiased var, n)} in training."""
    stats, margin = {}, float("inf")
    pad = (m - 1) // 2

    def conv(h, names):
        return torch.cat([F.conv1d(h, sd[k + ".weight"], sd[k + ".bias"],
                                   padding=sd[k + ".weight"].shape[2] // 2) for k in names], dim=1)

    hs = [conv(x[s:s + 1, :n].unsqueeze(1), ["embedding"]) for s, n in enumerate(lens)]
    hs = [conv(h, ["channel1_1", "channel2_1", "channel3_1"]) for h in hs]
    hs = _bn(hs, sd, "bn1", training, eps, stats)
    margin = min([margin] + [float(h.detach().abs().min()) for h in hs])
    hs = [F.leaky_relu(h, slope) for h in hs]
    for h in hs:
        hp = F.pad(h.detach(), (pad, pad), value=float("-inf"))
        margin = min(margin, _gap(hp.unfold(2, m, m - 1), 3))
    hs = [F.max_pool1d(h, m, stride=m - 1, padding=pad) for h in hs]
    hs = [conv(h, ["channel1_2", "channel2_2", "channel3_2"]) for h in hs]
    hs = _bn(hs, sd, "bn2", training, eps, stats)
    margin = min([margin] + [float(h.detach().abs().min()) for h in hs])
    hs = [F.leaky_relu(h, slope) for h in hs]
    margin = min([margin] + [_gap(h.detach(), 2) for h in hs])
    if info is not None:
        info["margin"], info["stats"] = margin, stats
    return torch.cat([torch.cat([h.max(dim=-1)[0], h.mean(dim=-1)], dim=-1) for h in hs])
