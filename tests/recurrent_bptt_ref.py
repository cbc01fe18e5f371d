"""The backward pass through time of the recurrent actor-critic's memory, written out from its formulas in torch float64: loops over t, no autograd.
What tests/test_recurrent_bptt.py checks against autograd and tests/test_recurrent_bptt_gpu.py compares the device kernels against
(csrc/recurrent_bptt.h).  The forward half is tests/recurrent_ref.py's cell, kept with its gate activations.

    gates = x W_ih^T + b_ih + h W_hh^T + b_hh        rows in torch's order i, f, g, o;  i, f, o = sigmoid, g = tanh;  c' = f c + i g;  h' = o tanh(c')

    backward, carries dh_rec = dc_rec = 0, t = T-1 .. 0:
        dh  = dY[t] + dh_rec                  tc = tanh(c'[t])
        do~ = dh tc o(1-o)                    dc  = dc_rec + dh o (1 - tc^2)
        di~ = dc g i(1-i)    df~ = dc c_used[t] f(1-f)    dg~ = dc i (1 - g^2)           dG[t] = (di~, df~, dg~, do~)
        dh_rec = dG[t] W_hh,  dc_rec = dc f;  both zero on rows where reset[t] is set
    dW_ih = dG^T X,  dW_hh = dG^T h_used,  db_ih = db_hh = the column sums of dG, over all T B rows
"""
import torch

from tests import recurrent_ref as ref


def resets_from_dones(dones, T, B):
    """reset [T][B] int64 of the first T slots and B environments of a done pattern [T'][N'][1]: reset[0] = 0, reset[t] = dones[t-1]."""
    reset = torch.zeros(T, B, dtype=torch.long)
    reset[1:] = dones[:T - 1, :B, 0] != 0
    return reset


def forward(xs, reset, h0, c0, params):
    """The roll with everything the backward pass reads, float64: dict of i, f, g, o, c_new, h_new, h_used, c_used, each [T][B][H]."""
    w_ih, w_hh, b_ih, b_hh = (p.detach().double() for p in params)
    H = w_hh.shape[1]
    h, c = h0.detach().double(), c0.detach().double()
    keep = {k: [] for k in ("i", "f", "g", "o", "c_new", "h_new", "h_used", "c_used")}
    for t in range(xs.shape[0]):
        if reset is not None:
            live = (reset[t] == 0).double().unsqueeze(1)
            h, c = h * live, c * live
        gates = xs[t].detach().double() @ w_ih.T + b_ih + h @ w_hh.T + b_hh
        i, f, o = (ref.sigmoid(gates[:, k * H:(k + 1) * H]) for k in (0, 1, 3))
        g = torch.tanh(gates[:, 2 * H:3 * H])
        c1 = f * c + i * g
        h1 = o * torch.tanh(c1)
        for k, v in (("i", i), ("f", f), ("g", g), ("o", o), ("c_new", c1), ("h_new", h1), ("h_used", h), ("c_used", c)):
            keep[k].append(v)
        h, c = h1, c1
    return {k: torch.stack(v) for k, v in keep.items()}


def backward(dY, fwd, reset, w_hh):
    """dG [T][B][4H] float64 from dY [T][B][H] and ``forward``'s dict."""
    w_hh = w_hh.detach().double()
    T, B, H = fwd["i"].shape
    dh_rec, dc_rec = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
    dG = [None] * T
    for t in range(T - 1, -1, -1):
        i, f, g, o = (fwd[k][t] for k in "ifgo")
        dh = dY[t].detach().double() + dh_rec
        tc = torch.tanh(fwd["c_new"][t])
        d_o = dh * tc * (o * (1 - o))
        dc = dc_rec + dh * o * (1 - tc * tc)
        d_i = dc * g * (i * (1 - i))
        d_f = dc * fwd["c_used"][t] * (f * (1 - f))
        d_g = dc * i * (1 - g * g)
        dG[t] = torch.cat((d_i, d_f, d_g, d_o), dim=1)
        dh_rec, dc_rec = dG[t] @ w_hh, dc * f
        if reset is not None:
            live = (reset[t] == 0).double().unsqueeze(1)
            dh_rec, dc_rec = dh_rec * live, dc_rec * live
    return torch.stack(dG)


def weight_grads(dG, xs, h_used):
    """(dW_ih [4H][I], dW_hh [4H][H], db [4H]) over all T B rows."""
    g2 = dG.flatten(0, 1)
    return g2.T @ xs.detach().double().flatten(0, 1), g2.T @ h_used.flatten(0, 1), g2.sum(0)


def grads(xs, reset, h0, c0, params, dY):
    """Everything at once -> dict of dW_ih, dW_hh, db, dG and the forward's y."""
    fwd = forward(xs, reset, h0, c0, params)
    dG = backward(dY, fwd, reset, params[1])
    dW_ih, dW_hh, db = weight_grads(dG, xs, fwd["h_used"])
    return {"dW_ih": dW_ih, "dW_hh": dW_hh, "db": db, "dG": dG, "y": fwd["h_new"], "c_last": fwd["c_new"][-1]}


def autograd_grads(xs, reset, h0, c0, params, dY, dtype):
    """The same quantities from torch autograd through a loop of lstm_cell's expressions in ``dtype`` on the CPU (dG[t] is the gradient of the gate
    pre-activations of step t) -> dict as ``grads``."""
    w_ih, w_hh, b_ih, b_hh = (p.detach().to(dtype).clone().requires_grad_(True) for p in params)
    H = w_hh.shape[1]
    h, c = h0.detach().to(dtype), c0.detach().to(dtype)
    x = xs.detach().to(dtype)
    pre, ys = [], []
    for t in range(x.shape[0]):
        if reset is not None:
            live = (reset[t] == 0).to(dtype).unsqueeze(1)
            h, c = h * live, c * live
        gates = torch.nn.functional.linear(x[t], w_ih, b_ih) + torch.nn.functional.linear(h, w_hh, b_hh)
        gates.retain_grad()
        pre.append(gates)
        i, f, g, o = gates.chunk(4, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        ys.append(h)
    y = torch.stack(ys)
    (y * dY.detach().to(dtype)).sum().backward()
    assert torch.equal(b_ih.grad, b_hh.grad)
    return {"dW_ih": w_ih.grad, "dW_hh": w_hh.grad, "db": b_ih.grad, "dG": torch.stack([p.grad for p in pre]), "y": y.detach(), "c_last": c.detach()}
