"""Restatement of the DEMO brain model's temporal front end and head
(HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:474-515 Inception1D, :250-399
HL_HGAT_attpool) on top of oracle.hodge_ref, for the tests of
tests/test_brain_head.py: plain torch on the CPU, fp32 or fp64
(``.double()``), state_dict compatible with the product classes.

The front end is written channels-last, as the HIP kernels see it: a
convolution is a sum over taps of row-shifted matrix products, the max-pool a
max over strided windows of the -inf padded series.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import hodge_ref as R


def conv_time(x, weight, bias):
    """x [N, T, Cin], weight [Cout, Cin, taps] (nn.Conv1d layout), zero padding
    taps // 2 at both ends of every series -> [N, T, Cout]."""
    taps = weight.shape[-1]
    half = taps // 2
    T = x.shape[1]
    xp = F.pad(x, (0, 0, half, half))
    y = sum(torch.einsum("ntc,oc->nto", xp[:, k:k + T], weight[:, :, k]) for k in range(taps))
    return y if bias is None else y + bias


def leaky_maxpool_time(x, slope, m):
    """MaxPool1d(m, stride=m-1, padding=(m-1)//2) of LeakyReLU(slope)(x) over
    axis 1 of x [N, T, C]."""
    s, p = m - 1, (m - 1) // 2
    h = F.pad(F.leaky_relu(x, slope), (0, 0, p, p), value=float("-inf"))
    return h.unfold(1, m, s).max(dim=-1)[0]


def time_readout(x, slope):
    h = F.leaky_relu(x, slope)
    return torch.cat([h.max(dim=1)[0], h.mean(dim=1)], dim=-1)


class RefInception1D(nn.Module):
    def __init__(self, in_channels=64, num_channels=8, maxpool=3, if_dim_reduction=False,
                 leaky_slope=0.1, if_readout=False):
        super().__init__()
        c, n = in_channels, num_channels
        self.maxpool, self.slope, self.if_readout = maxpool, leaky_slope, if_readout
        self.embedding = nn.Conv1d(1, c, 5, padding=2)
        self.channel1_1 = nn.Conv1d(c, int(c / 4), 1)
        self.channel2_1 = nn.Conv1d(c, int(c / 2), 3, padding=1)
        self.channel3_1 = nn.Conv1d(c, int(c / 4), 5, padding=2)
        self.channel1_2 = nn.Conv1d(c, n, 1)
        self.channel2_2 = nn.Conv1d(c, n * 2, 3, padding=1)
        self.channel3_2 = nn.Conv1d(c, n, 5, padding=2)
        self.bn1 = nn.BatchNorm1d(c)
        self.bn2 = nn.BatchNorm1d(n * 4)

    @staticmethod
    def _branches(x, convs):
        return torch.cat([conv_time(x, c.weight, c.bias) for c in convs], dim=-1)

    @staticmethod
    def _bn(x, bn):
        return bn(x.reshape(-1, x.shape[-1])).view(x.shape)

    def pre_activations(self, x):
        """(bn1 output, bn2 output): the values the two LeakyReLUs see."""
        h = conv_time(x.unsqueeze(-1), self.embedding.weight, self.embedding.bias)
        z1 = self._bn(self._branches(h, (self.channel1_1, self.channel2_1, self.channel3_1)),
                      self.bn1)
        h = leaky_maxpool_time(z1, self.slope, self.maxpool)
        z2 = self._bn(self._branches(h, (self.channel1_2, self.channel2_2, self.channel3_2)),
                      self.bn2)
        return z1, z2

    def forward(self, x):
        _, z2 = self.pre_activations(x)
        if self.if_readout:
            return time_readout(z2, self.slope)
        return F.leaky_relu(z2, self.slope)


class RefDemoConv(nn.Module):
    """HodgeLaguerreFastConv as published (oracle: laguerre_fast_conv_demo)."""

    def __init__(self, cin, cout, K):
        super().__init__()
        self.lins = nn.ModuleList([R.RefPygLinear(cin, cout) for _ in range(K)])
        self.bias = nn.Parameter(torch.zeros(cout))

    def forward(self, x, adj):
        ei, ew = adj
        return R.laguerre_fast_conv_demo(x, ei, ew.to(x.dtype), [l.weight for l in self.lins],
                                         self.bias)


def _block(cin_t, cin_s, cout, K, slope=0.1):
    layers = [(RefDemoConv(cin_t, cout, K), "x_t, adj_t -> x_t"),
              (R.RefBatchNorm(cout), "x_t -> x_t"),
              (nn.LeakyReLU(slope), "x_t -> x_t"),
              (nn.Dropout(0.0), "x_t -> x_t"),
              (RefDemoConv(cin_s, cout, K), "x_s, adj_s -> x_s"),
              (R.RefBatchNorm(cout), "x_s -> x_s"),
              (nn.LeakyReLU(slope), "x_s -> x_s"),
              (nn.Dropout(0.0), "x_s -> x_s"),
              (lambda a, b: [a, b], "x_t, x_s -> x")]
    return R.RefSequential("x_t, adj_t, x_s, adj_s", layers)


def _ahead(counts):
    c = torch.as_tensor(counts).view(-1).to(torch.long)
    return torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.long), c]), 0)[:-1]


class RefBrainHead(nn.Module):
    def __init__(self, channels=[2, 2, 2], filters=[32, 64, 128], mlp_channels=[], K=4,
                 node_dim=64, edge_dim=1, num_classes=1, pool_num=2, num_nodepedge=2089):
        super().__init__()
        self.channels, self.mlp_channels, self.pool_num = channels, mlp_channels, pool_num
        self.node_embedding = RefInception1D(if_readout=True)
        c0 = filters[0]
        self.HL_init_conv = _block(node_dim, edge_dim, c0, K)
        gin = last = c0
        for i, gout in enumerate(filters):
            for j in range(channels[i]):
                setattr(self, f"NEInt{i}{j}", R.RefNodeEdgeInt(d=gin, dv=gout))
                setattr(self, f"NEConv{i}{j}", _block(gout, gout, gout, K))
                gin, last = gin + gout, gout
            if i < pool_num:
                setattr(self, f"NEAtt{i}", R.RefNodeEdgeInt(d=gin, dv=gout, only_att=True))
        self.readout = R.RefSequential("x_t, adj_t, x_s, adj_s", [
            (RefDemoConv(last, 1, 1), "x_t, adj_t -> x_t"),
            (RefDemoConv(last, 1, 1), "x_s, adj_s -> x_s"),
            (lambda a, b: [a, b], "x_t, x_s -> x")])
        mlp_in = num_nodepedge
        for i, mo in enumerate(mlp_channels):
            setattr(self, f"mlp{i}", nn.Sequential(nn.Linear(mlp_in, mo), nn.BatchNorm1d(mo),
                                                   nn.LeakyReLU(0.1), nn.Dropout(0.0)))
            mlp_in = mo
        self.out = nn.Linear(mlp_in, num_classes)

    @staticmethod
    def _graph(d, n_t, n_s):
        par = R.adj2par1(d.edge_index, n_t, n_s)
        return par, R.degree(d.edge_index.reshape(-1), num_nodes=n_t) + 1e-6

    def forward(self, datas):
        d = datas[0]
        G = torch.as_tensor(d.num_node1).numel()
        x_t = self.node_embedding(d.x_t)
        adj_t, adj_s = (d.edge_index_t, d.edge_weight_t), (d.edge_index_s, d.edge_weight_s)
        x_t, x_s = self.HL_init_conv(x_t, adj_t, d.x_s, adj_s)
        x_t0, x_s0 = x_t, x_s
        par, D = self._graph(d, x_t0.shape[0], x_s0.shape[0])
        node_att = edge_att = None
        k = 0
        for i in range(len(self.channels)):
            for j in range(self.channels[i]):
                x_t, x_s = getattr(self, f"NEInt{i}{j}")(x_t0, x_s0, par, D)
                x_t, x_s = getattr(self, f"NEConv{i}{j}")(x_t, adj_t, x_s, adj_s)
                x_t0 = torch.cat([x_t0, x_t], -1)
                x_s0 = torch.cat([x_s0, x_s], -1)
            if i < self.pool_num:
                a_t, a_s = getattr(self, f"NEAtt{i}")(x_t0, x_s0, par, D)
                if k == 0:
                    node_att, edge_att = a_t.view(G, -1), a_s.view(G, -1)
                fine, coarse = datas[k], datas[k + 1]
                # cluster of every fine row, shifted to its graph's coarse rows
                pos_t = fine.pos_t.view(-1) + torch.repeat_interleave(
                    _ahead(coarse.num_node1), torch.as_tensor(fine.num_node1).view(-1))
                pos_s = fine.pos_s.view(-1) + torch.repeat_interleave(
                    _ahead(coarse.num_edge1), torch.as_tensor(fine.num_edge1).view(-1))
                kt, ks = ~torch.isinf(pos_t), ~torch.isinf(pos_s)
                x_t0 = R.scatter_mean((x_t0 * a_t)[kt], pos_t[kt].to(torch.long),
                                      coarse.x_t.shape[0])
                x_s0 = R.scatter_mean((x_s0 * a_s)[ks], pos_s[ks].to(torch.long),
                                      coarse.x_s.shape[0])
                adj_t = (coarse.edge_index_t, coarse.edge_weight_t)
                adj_s = (coarse.edge_index_s, coarse.edge_weight_s)
                k += 1
                par, D = self._graph(coarse, x_t0.shape[0], x_s0.shape[0])
        x_t, x_s = self.readout(x_t, adj_t, x_s, adj_s)
        x = torch.cat([x_s.view(G, -1), x_t.view(G, -1)], -1)
        for i in range(len(self.mlp_channels)):
            x = getattr(self, f"mlp{i}")(x)
        return self.out(x), x, node_att, edge_att
