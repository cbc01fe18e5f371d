"""The recurrent actor-critic's memory restated from its formulas in torch float64 (NOT nn.LSTM), and a plain Python loop version of rsl_rl's
split / pad of trajectories: what tests/test_recurrent.py and tests/test_recurrent_gpu.py compare rl_mpc_locomotion_amd.recurrent and the cell
kernel against.

    gates = x W_ih^T + b_ih + h W_hh^T + b_hh        W_ih [4H][I], W_hh [4H][H], rows in torch's order i, f, g, o
    i, f, o = sigmoid, g = tanh;   c' = f c + i g;   h' = o tanh(c')
"""
import torch

T_CASE, N_CASE = 6, 5


def done_patterns():
    """The done patterns of the CPU tests, [T=6][N=5][1] float32 each: 'mixed' has a done at t = 0 (environment 0), one at t = T - 1 (1), two
    consecutive ones (2), an environment with none (3) and one in the middle (4); 'all_early' gives every environment a done before T - 1, the
    case rsl_rl v1.0.2's unpad fails on; 'none' and 'all' are the two ends."""
    T, N = T_CASE, N_CASE
    mixed = torch.zeros(T, N, 1)
    mixed[0, 0], mixed[T - 1, 1], mixed[2, 2], mixed[3, 2], mixed[1, 4] = 1, 1, 1, 1, 1
    early = torch.zeros(T, N, 1)
    for e, t in enumerate((0, 1, 2, 3, 4)):
        early[t, e] = 1
    return {"mixed": mixed, "all_early": early, "none": torch.zeros(T, N, 1), "all": torch.ones(T, N, 1)}


def sigmoid(v):
    return 1.0 / (1.0 + torch.exp(-v))


def cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """One step, every argument converted to float64 -> (h', c')."""
    x, h, c, w_ih, w_hh, b_ih, b_hh = (t.detach().double() for t in (x, h, c, w_ih, w_hh, b_ih, b_hh))
    H = h.shape[1]
    gates = x @ w_ih.T + b_ih + h @ w_hh.T + b_hh
    i, f, g, o = (gates[:, k * H:(k + 1) * H] for k in range(4))
    c1 = sigmoid(f) * c + sigmoid(i) * torch.tanh(g)
    return sigmoid(o) * torch.tanh(c1), c1


def roll(xs, resets, h0, c0, params):
    """T steps: xs [T][n][I]; resets [T][n] (non-zero: the state of that row is zero before step t) or None; -> (h' [T][n][H], c' [T][n][H],
    the state each step started from after the zeroing: h [T][n][H], c [T][n][H]), float64."""
    h, c = h0.detach().double(), c0.detach().double()
    hs, cs, sh, sc = [], [], [], []
    for t in range(xs.shape[0]):
        if resets is not None:
            keep = (resets[t] == 0).double().unsqueeze(1)
            h, c = h * keep, c * keep
        sh.append(h); sc.append(c)
        h, c = cell(xs[t], h, c, *params)
        hs.append(h); cs.append(c)
    return torch.stack(hs), torch.stack(cs), torch.stack(sh), torch.stack(sc)


def elu(v):
    return torch.where(v > 0, v, torch.expm1(v))


def mlp(x, linears):
    """A Linear / ELU stack in float64; linears: [(weight, bias)]."""
    x = x.double()
    for k, (w, b) in enumerate(linears):
        x = x @ w.detach().double().T + b.detach().double()
        if k + 1 < len(linears):
            x = elu(x)
    return x


def split_and_pad_loop(tensor, dones):
    """The split / pad as loops: every environment's column, environment by environment, is cut after each done and after its last slot; every
    piece becomes a column of ``padded`` [T][n_traj][F], zero beyond its length; ``masks`` [T][n_traj] marks the piece.  Also returns, per
    trajectory, (environment, first step)."""
    T, N = tensor.shape[0], tensor.shape[1]
    pieces, where = [], []
    for e in range(N):
        start = 0
        for t in range(T):
            if t == T - 1 or float(dones[t, e, 0]) != 0.0:
                pieces.append(tensor[start:t + 1, e])
                where.append((e, start))
                start = t + 1
    padded = torch.zeros((T, len(pieces)) + tuple(tensor.shape[2:]), dtype=tensor.dtype)
    masks = torch.zeros((T, len(pieces)), dtype=torch.bool)
    for k, p in enumerate(pieces):
        padded[:len(p), k] = p
        masks[:len(p), k] = True
    return padded, masks, where
