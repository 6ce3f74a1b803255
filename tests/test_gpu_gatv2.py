"""GPU: the MaxK GATv2 kernels, their autograd Functions and MaxKGATv2Conv against the float64
restatements of tests/gatv2.py, within the derived bounds of include/maxk_hip.h ("MaxK GATv2
attention"). The 600-row graph of tests/gat_heads.py has row and column lengths on both sides of
every limit, a hub row of 5,000 and a hub column of 3,000 edges; its 33 x 700 graph (and the
transposed one) puts two hubs into one tile. Outputs are pre-filled with NaN and the scratch is
dirty: whatever a kernel fails to write fails the comparison.

Worst error / bound figures print with -s."""
import functools

import numpy as np
import pytest
import torch

import gat_heads as gh
import gatv2 as gv
import maxk_kernels as mk
from maxk_kernels import ops

pytestmark = pytest.mark.gpu

GRAPHS = {"main": (gh.graph_arrays, gh.NUM), "tile": (gh.tile_graph, gh.TILE_COLS),
          "tile_t": (gh.tile_graph_t, gh.TILE_ROWS)}
CASES = [(s, "main") for s in gv.SHAPES] + \
    [(s, g) for s in ((64, 4, 16), (256, 4, 255)) for g in ("tile", "tile_t")]


def dev_of(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


@functools.lru_cache(maxsize=None)
def case(shape, graph):
    """The host side of a case, computed once: structure, inputs, float64 results."""
    D, H, k = shape
    (ptr, idx), num_cols = GRAPHS[graph][0](), GRAPHS[graph][1]
    tr = gh.transposed(ptr, idx, num_cols)
    ins = gv.inputs(ptr.size - 1, num_cols, idx.size, D, H, k, seed=D + H + k)
    return (ptr, idx) + tr, ins, gv.score64(ptr, idx, *ins[:4]), gv.backward64(ptr, idx, *ins)


def on_device(shape, graph, dev):
    st, ins, fwd64, bwd64 = case(shape, graph)
    return [dev_of(a, dev) for a in st], [dev_of(a, dev) for a in ins], fwd64, bwd64


def launch(st, ins, need=(True, True, True)):
    """The score forward and both backward halves into NaN-filled outputs, with a dirty scratch."""
    ptr, idx, pt, it, order = st
    data, sel, fd, attn, g = ins
    dev, (H, E), (n, D) = ptr.device, g.shape, fd.shape
    delta = ops.gatv2_score(ptr, idx, data, sel, fd, attn, gv.SLOPE, out=nan(dev, H, E))
    scratch = torch.full((ops.gatv2_scratch_bytes(n, D),), 0xFF, dtype=torch.uint8, device=dev)
    gfd, gattn = ops.gatv2_score_backward_rows(ptr, idx, data, sel, fd, attn, gv.SLOPE, g,
                                               out=(nan(dev, n, D), nan(dev, *attn.shape)),
                                               scratch=scratch)
    gsp = ops.gatv2_score_backward_cols(pt, it, order, data, sel, fd, attn, gv.SLOPE, g,
                                        out=nan(dev, *data.shape))
    return delta, gsp, gfd, gattn


@pytest.mark.parametrize("shape,graph", CASES)
def test_score_forward_and_backward_within_the_bounds(gpu, shape, graph):
    st, ins, (delta, dmag, dm), (sp, gfd, gat) = on_device(shape, graph, gpu)
    got = [t.cpu().numpy() for t in launch(st, ins)]
    lengths = np.diff(st[0].cpu().numpy())
    reg = np.repeat([gh.regime(int(n)) for n in lengths], lengths)
    for r in sorted(set(reg.tolist())):
        w = gv.worst(got[0][:, reg == r], delta[:, reg == r], dmag[:, reg == r], dm[:, reg == r])
        print(f"\n{shape} {graph} Delta, regime {r}: worst error / bound {w:.3f}")
        assert w <= 1.0
    for name, g, (want, mag, m) in (("grad_sp", got[1], sp), ("grad_fd", got[2], gfd),
                                    ("grad_attn", got[3].reshape(-1), gat)):
        w = gv.worst(g, want, mag, m)
        print(f"{shape} {graph} {name}: worst error / bound {w:.3f}")
        assert w <= 1.0, name


def strided(t, stride):
    buf = torch.zeros((t.shape[0], stride), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


@pytest.mark.parametrize("shape", [(64, 4, 16), (256, 4, 255)])
def test_row_strided_tables_give_the_same_bits(gpu, shape):
    """data_stride, index_stride above k and fd_stride above D, read in place."""
    (D, _, k), (st, ins, _, _) = shape, on_device(shape, "main", gpu)
    data, sel, fd = strided(ins[0], k + 3), strided(ins[1], k + 5), strided(ins[2], D + 4)
    assert not (data.is_contiguous() or sel.is_contiguous() or fd.is_contiguous())
    for got, want in zip(launch(st, [data, sel, fd] + ins[3:]), launch(st, ins)):
        assert torch.equal(got, want)


def test_softmax_heads_is_the_single_head_kernel_per_row(gpu):
    ptr = dev_of(gh.graph_arrays()[0], gpu)
    E = int(ptr[-1])
    x, gy = (torch.randn(3, E, device=gpu, generator=torch.Generator(gpu).manual_seed(s)) * 3
             for s in (1, 2))
    y = ops.edge_softmax_heads(ptr, x, out=nan(gpu, 3, E))
    gx = ops.edge_softmax_backward_heads(ptr, y, gy, out=nan(gpu, 3, E))
    for h in range(3):
        assert torch.equal(y[h], ops.edge_softmax(ptr, x[h].contiguous()))
        assert torch.equal(gx[h], ops.edge_softmax_backward(ptr, y[h].contiguous(),
                                                            gy[h].contiguous()))


def test_one_captured_replay_with_swapped_inputs_equals_eager(gpu):
    st, ins, _, _ = on_device((256, 8, 32), "main", gpu)
    static = [t.clone() for t in ins]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        launch(st, static)  # warm up: code objects loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = launch(st, static)
    fresh = [torch.roll(t, 1, 0) if t.dtype == torch.float32 else t for t in ins]
    for s, f in zip(static, fresh):
        s.copy_(f)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, launch(st, fresh)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("need", [(True, True, True), (True, False, False), (False, False, True)])
def test_function_gradients_within_the_bounds(gpu, need):
    shape = (256, 8, 32)
    st, ins, _, _ = on_device(shape, "main", gpu)
    data, sel, fd, attn, w = ins
    leaves = [t.clone().requires_grad_(r) for t, r in zip((data, fd, attn), need)]
    graph = mk.CSRGraph(st[0], st[1])
    alpha = mk.gatv2_attention(graph, leaves[0], sel, leaves[1], leaves[2], gv.SLOPE)
    assert torch.equal(alpha, ops.edge_softmax_heads(
        st[0], ops.gatv2_score(st[0], st[1], data, sel, fd, attn, gv.SLOPE)))
    (alpha * w).sum().backward()
    g = ops.edge_softmax_backward_heads(st[0], alpha.detach(), w)
    host = case(shape, "main")
    refs = gv.backward64(host[0][0], host[0][1], *host[1][:4], g.cpu().numpy())
    for leaf, r, (want, mag, m) in zip(leaves, need, refs):
        assert (leaf.grad is not None) == r
        if r:
            assert gv.worst(leaf.grad.cpu().numpy().reshape(want.shape), want, mag, m) <= 1.0


def close(got, want, what):
    got, want = got.detach().double().cpu(), want.detach()
    rel = float((got - want).norm() / want.norm())
    print(f"\n{what}: relative error {rel:.2e}")
    assert rel <= 1e-5, what


@pytest.mark.parametrize("in_feats,F_,H,k,share", [(24, 8, 4, 32, False), (24, 8, 4, 32, True),
                                                   (40, 32, 8, 32, False)])
def test_layer_against_the_float64_model(gpu, in_feats, F_, H, k, share):
    """k = D: dglnn.GATv2Conv's dense formula; k < D: the model with the layer's own sp_index.
    Features are multiples of 1/4 and the linear layers' parameters of 1/16, so fs and fd are the
    same numbers in f32 and in float64 and lrelu' takes the same branch in both: with rounded fs
    and fd a sum within an ulp of zero flips the branch of one (edge, feature) pair, which moves
    the fc gradients by 2e-4 norm-wise in a plain f32 torch composition as well."""
    ptr, idx = gh.graph_arrays()
    torch.manual_seed(k + H)
    layer = mk.MaxKGATv2Conv(in_feats, F_, H, maxk=k, share_weights=share,
                             allow_zero_in_degree=True).to(gpu)
    torch.nn.init.normal_(layer.fc_src.bias)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if name != "attn":
                p.copy_(torch.round(p * 16) / 16)
    feat = torch.randint(-8, 9, (gh.NUM, in_feats), device=gpu) / 4
    out = layer(mk.CSRGraph(dev_of(ptr, gpu), dev_of(idx, gpu)), feat)
    assert out.shape == (gh.NUM, H, F_)
    wout = torch.randn_like(out)
    (out * wout).sum().backward()
    names = ["fc_src.weight", "fc_src.bias", "attn"] + ([] if share else ["fc_dst.weight",
                                                                           "fc_dst.bias"])
    params = dict(layer.named_parameters())
    p = {n: params[n].detach().double().cpu().requires_grad_(True) for n in names}
    dst = "fc_src" if share else "fc_dst"
    p64 = {"w_src": p["fc_src.weight"], "b_src": p["fc_src.bias"], "w_dst": p[dst + ".weight"],
           "b_dst": p[dst + ".bias"], "attn": p["attn"]}
    sp_index = None if k == H * F_ else mk.maxk(layer.fc_src(feat), k)[1].cpu()
    ref = gv.model64(ptr, idx, feat.double().cpu(), p64, H, sp_index)
    (ref * wout.double().cpu()).sum().backward()
    close(out, ref, "out")
    for n in names:
        close(params[n].grad, p[n].grad, n)
