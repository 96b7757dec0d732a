"""MOSRGNN on the gfx950 kernels: bit identity with SRGNN's launches (loss, the 17 gradients, the dense dE against the sparse table
gradient scattered), the head without the tower against the float64 restatement, one row per node slot against the batch-wide
dedup, the model against the fixture of the reference's own MOSRGNN in both input forms (loss, all 27 gradients, compute_item,
predict, the fused top-k), determinism, bad positions, the optimizer's two groups, and main.py end to end.  Every test here needs
the new class, so each fails without the feature."""
import os

import numpy as np
import pytest
import torch

from pixelrec_amd import ops
from tests import mosrgnn_restate as R
from tests import srgnn_restate as SR
from tests.mo_common import GOLD, assert_optimizer_state_round_trips, assert_two_fresh_models_agree, bits as _bits, my_name, run_main_py
from tests.test_mosrgnn_cpu import _config, build_from_fixture

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24
SEG_SHORT = 8                      # csrc/embed_grad.hip: a longer segment takes the staged branch of the segment sum


# ------------------------------------------------------------------------------------------------------------ cases
def _block_model(D, L, step, seed=0):
    import pixelrec_amd.model as M

    class DL:
        item_num = 13

    torch.manual_seed(seed)
    return M.MOSRGNN(_config(D, L, step, 37), DL()).cuda().train()


def _sessions(B, L, M, seed):
    """(item_seq [B, L] right-padded, target [B, 2]) positions in [1, M - 1) -- row M - 1 is read by nobody: session 0 is full
    length with L distinct items (no padding node), session 1 has one item, the others 2..L items with revisits as they fall; item
    7 is a node of the first min(B, 12) sessions (a segment longer than SEG_SHORT at B = 16); session 2's negative is a node of
    session 0, session 3's positive a node of session 0."""
    rng = np.random.default_rng(seed)
    hot = 7
    seq = np.zeros((B, L), dtype=np.int64)
    others = np.array([i for i in range(1, M - 1) if i != hot])
    seq[0] = np.concatenate(([hot], rng.choice(others, size=L - 1, replace=False)))
    seq[1, 0] = hot
    for b in range(2, B):
        n = int(rng.integers(2, L + 1))
        seq[b, :n] = rng.integers(1, M - 1, size=n)
        if b < 12:
            seq[b, int(rng.integers(0, n))] = hot
        else:
            seq[b][seq[b] == hot] = hot + 1
    tgt = rng.integers(1, M - 1, size=(B, 2))
    tgt[2, 1], tgt[3, 0] = seq[0, 1], seq[0, 2]
    for b in range(B):
        while tgt[b, 0] == tgt[b, 1]:
            tgt[b, int(b != 2)] = rng.integers(1, M - 1)
    assert (seq[0] != 0).all() and len(set(seq[0].tolist())) == L and (seq[1] != 0).sum() == 1
    return seq, tgt


def _weights(m, dtype, device="cpu"):
    return {k: m.get_parameter(k).detach().to(device=device, dtype=dtype).clone() for k in R.NAMES}


def _grads17(m):
    return {k: m.get_parameter(k).grad.detach().clone() for k in R.NAMES}


SHAPES = [(6, 5, 12, 20, 1), (6, 5, 12, 20, 2), (16, 10, 64, 61, 2)]       # (B, L, D, M, step)


def _case(B, L, D, M, step):
    m = _block_model(D, L, step)
    seq, tgt = _sessions(B, L, M, 7 * B + L)
    E = (torch.randn(M, D, generator=torch.Generator().manual_seed(D + B)) * 0.5).cuda()
    return m, seq, tgt, E


# ------------------------------------------------------------------------------------------------------------ 1. SRGNN's launches
def _srgnn_like(m, E):
    """An SRGNN whose weights are MOSRGNN m's and whose table is E (item id j reads E[j])."""
    from pixelrec_amd.model import SRGNN

    class DL:
        item_num = E.shape[0]

    s = SRGNN({"embedding_size": m.hidden_size, "step": m.step, "MAX_ITEM_LIST_LENGTH": m.max_seq_length}, DL())
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items() if not k.startswith("visual_encoder.")}
    sd["embedding.weight"] = E.detach().cpu()
    s.load_state_dict(sd, strict=True)
    return s.cuda().train()


@pytest.mark.parametrize("B,L,D,M,step", SHAPES)
def test_step_is_srgnns_bit_for_bit(B, L, D, M, step, monkeypatch):
    """An SRGNN with item_num = M, table E and MOSRGNN's weights on the same rows goes through the same launches: the same loss
    bits and 17 gradient bits, and its sparse table gradient scattered into zeros IS dE -- +0.0 on row 0 and on rows nobody reads,
    in a block that held NaN before the dense sink ran, under the (3L, 0, L, 2L) layout of the graph build's id rows."""
    m, seq, tgt, E = _case(B, L, D, M, step)
    if B == 16:
        cnt = np.bincount(np.concatenate([np.unique(r) for r in seq]), minlength=M)
        assert cnt[7] == 12 > SEG_SHORT
    real, layouts = ops.seq_occ_dense_grad, []

    def into_nan(items, layout, dx0, out, coef, n_rows, d_rows=None, ws=None):
        layouts.append(tuple(layout))
        block = torch.full((n_rows, out.shape[2]), float("nan"), device=out.device)
        return real(items, layout, dx0, out, coef, n_rows, d_rows=block, ws=ws)

    monkeypatch.setattr(ops, "seq_occ_dense_grad", into_nan)
    E = E.requires_grad_(True)
    sd, td = torch.from_numpy(seq).cuda(), torch.from_numpy(tgt).cuda()
    loss = m.loss_from_embeddings(E, sd, td)
    loss.backward()
    assert layouts == [(3 * L, 0, L, 2 * L)]
    s = _srgnn_like(m, E)
    loss_s = s((sd, (sd != 0).long(), td))
    loss_s.backward()
    ops.raise_on_bad_indices()
    assert torch.equal(_bits(loss.detach()), _bits(loss_s.detach()))
    for k in R.NAMES:
        a, b = m.get_parameter(k).grad, s.get_parameter(k).grad
        assert float(a.abs().max()) > 0 and torch.equal(_bits(a), _bits(b)), k
    assert m.gnn.linear_edge_f.weight.grad is None
    dE = E.grad
    assert torch.equal(_bits(dE), _bits(s.sparse_table_grad.to_dense(M)))
    read = torch.zeros(M, dtype=torch.bool, device="cuda")
    read[sd.view(-1)] = True
    read[td.view(-1)] = True
    read[0] = False
    assert not bool(read[M - 1]) and int(_bits(dE[~read]).abs().max()) == 0 and float(dE[read].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ 2. the head alone
def _assert_grads(tag, got, g64, g32, names):
    for k in names:
        err, d32 = float((got[k].double().cpu() - g64[k]).abs().max()), float((g32[k].double() - g64[k]).abs().max())
        big = float(g64[k].abs().max())
        print(tag, "grad", k, "err", err, "float32 restatement", d32, "largest entry", big)
        assert err <= 2 * d32 + 1e-6 * big, k


@pytest.fixture(scope="module")
def head_cases():
    """{shape: (model, seq, tgt, E, float64 and float32 restatement results)}: each reference is computed once."""
    cache = {}

    def get(shape):
        if shape not in cache:
            B, L, D, M, step = shape
            m, seq, tgt, E = _case(B, L, D, M, step)
            res = {dt: R.loss_and_grads(_weights(m, dt), E.detach().cpu().to(dt), seq, tgt, step) for dt in (torch.float64, torch.float32)}
            cache[shape] = (m, seq, tgt, E, res)
        return cache[shape]

    return get


@pytest.mark.parametrize("shape", [SHAPES[2], (16, 10, 512, 61, 2)])
def test_head_without_the_tower_matches_float64(head_cases, shape):
    """loss_from_embeddings on a random leaf E against mosrgnn_restate in float64, by test_gpu_modin.py's rule: the loss within
    2 |L32 - L64| + 2e-6 max(1, |L64|), every gradient (the 17 tensors and dE) within 2 d32 + 1e-6 max|g64|, L32 / d32 from the
    float32 restatement on the same inputs; the no_grad call gives the same loss bits; a detached E still drives the block's
    backward to the same 17 gradient bits."""
    m, seq, tgt, E, res = head_cases(shape)
    (L64, g64), (L32, g32) = res[torch.float64], res[torch.float32]
    L64, L32 = float(L64), float(L32)
    E = E.detach().clone().requires_grad_(True)
    sd, td = torch.from_numpy(seq).cuda(), torch.from_numpy(tgt).cuda()
    loss = m.loss_from_embeddings(E, sd, td)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    ops.raise_on_bad_indices()
    print("loss", float(loss.detach()), L64, "float32 restatement", L32)
    assert abs(float(loss.detach()) - L64) <= 2 * abs(L32 - L64) + 2e-6 * max(1.0, abs(L64))
    got = _grads17(m)
    got[R.E_KEY] = E.grad
    assert E.grad.shape == E.shape
    _assert_grads(shape, got, g64, g32, R.NAMES + [R.E_KEY])
    with torch.no_grad():
        again = m.loss_from_embeddings(E.detach(), sd, td)
    assert not again.requires_grad and torch.equal(_bits(again), _bits(loss.detach()))
    frozen = m.loss_from_embeddings(E.detach(), sd, td)
    assert frozen.requires_grad
    frozen.backward()
    for k in R.NAMES:                                               # the same step again: the same gradients
        assert torch.equal(_bits(m.get_parameter(k).grad), _bits(got[k])), k


# ------------------------------------------------------------------------------------------------------------ 3. the dedup
def _slot_form(m, seq, tgt, E):
    """The reference's one row per node slot and target, from rows of E: (Ex, graph dict, mask, target) as `_reference_form`
    builds them for the collate's graph at n = the batch's largest node count, plus the row of E behind every row of Ex[1:]."""
    B, L = seq.shape
    n = max(len(np.unique(r)) for r in seq)
    nodes, alias, A = SR.session_graph(seq, n)
    images = torch.zeros(B * (n + 2), 1, 1, 1, device="cuda")
    g, mask, target, _ = m._reference_form(torch.from_numpy(alias), torch.from_numpy(A).float(), torch.from_numpy((seq != 0).astype(np.int64)),
                                           images)
    flat = torch.from_numpy(np.concatenate((nodes, tgt), axis=1)).cuda().view(-1)
    return torch.cat((E.detach()[:1], E.detach()[flat])), g, mask, target, flat


@pytest.mark.parametrize("B,L,D,M,step", SHAPES[1:])
def test_dedup_does_not_change_the_function(B, L, D, M, step):
    """One row per node slot and target (the reference's form: row 1 + b (n + 2) + k holds a copy of E[nodes[b, k]]) against the
    batch-wide dedup: the same loss bits; dE[r] is the sum of its copies' gradients, in float64 within (k + 1) 2^-24 sum|terms|;
    the copies of row 0 (padding nodes) get exactly zero."""
    m, seq, tgt, E = _case(B, L, D, M, step)
    E = E.requires_grad_(True)
    loss = m.loss_from_embeddings(E, torch.from_numpy(seq).cuda(), torch.from_numpy(tgt).cuda())
    loss.backward()
    g17 = _grads17(m)
    Ex, g, mask, target, flat = _slot_form(m, seq, tgt, E)
    Ex = Ex.requires_grad_(True)
    loss_x = m._loss_from_graph(Ex, g, mask, target)
    loss_x.backward()
    ops.raise_on_bad_indices()
    assert torch.equal(_bits(loss_x.detach()), _bits(loss.detach()))
    terms = Ex.grad[1:].double()
    assert bool((flat == 0).any()) and float(terms[flat == 0].abs().max()) == 0 and float(Ex.grad[0].abs().max()) == 0
    z = lambda: torch.zeros(M, D, dtype=torch.float64, device="cuda")
    d64, dabs = z().index_add_(0, flat, terms), z().index_add_(0, flat, terms.abs())
    k = torch.zeros(M, dtype=torch.float64, device="cuda").index_add_(0, flat, torch.ones_like(flat, dtype=torch.float64))
    over = (E.grad.double() - d64).abs() - (k[:, None] + 1) * U32 * dabs
    print("dE against the summed copies", float((E.grad.double() - d64).abs().max()))
    assert float(over[1:].max()) <= 0 and float(E.grad[0].abs().max()) == 0
    for name in R.NAMES:                                            # the block saw the same rows: the same launches, the same bits
        assert torch.equal(_bits(m.get_parameter(name).grad), _bits(g17[name])), name


# ------------------------------------------------------------------------------------------------------------ 4. the fixture
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "mosrgnn_tiny.npz"))


def _inputs(g, j, store, form):
    seq, tgt = g[f"b{j}.item_seq"], g[f"b{j}.target"]
    if form == "positions":                                         # what MoGraphTrainBatcher.make_batch builds, then modal_inputs
        from pixelrec_amd.data.dataset import positions_into_distinct_images

        index, image_ids = positions_into_distinct_images(seq, tgt)
        return torch.from_numpy(index).cuda(), store[torch.from_numpy(image_ids).cuda()]
    slots = torch.from_numpy(np.concatenate((g[f"b{j}.nodes"], tgt), axis=1)).cuda()        # mograph_train_collate's 4-tuple
    return (torch.from_numpy(g[f"b{j}.alias"]).cuda(), torch.from_numpy(g[f"b{j}.A"]).cuda(), torch.from_numpy(g[f"b{j}.mask"]).cuda(),
            store[slots].flatten(0, 1))


def _step(m, g, j, store, form):
    loss = m(_inputs(g, j, store, form))
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad and p.grad is not None}


@pytest.mark.parametrize("form", ["positions", "reference"])
def test_model_matches_the_reference_fixture(gold, form):
    """Loss, all 27 gradients, compute_item and predict against the stored results of the reference's MOSRGNN for step 1 and 2,
    with the batch in the batcher's form and in the reference's 4-tuple.  Budgets: the project's recorded ones for this tiny tower
    (tests/test_gpu_modin.py) -- loss 3e-5 max(1, |loss|), gradients 5e-6 + 5e-4 max|g|, item features 3e-5, scores 1e-4 -- each
    plus the quantity's stored ref_err.  Then ops.score_topk on encode_last against predict + masks + topk."""
    g = gold
    store = torch.from_numpy(g["store"].astype(np.float32)).cuda()
    names = [str(k) for k in g["param.keys"]]
    win = torch.from_numpy(g["eval.windows"]).cuda()
    for step in (int(s) for s in g["steps"]):
        p = f"s{step}."
        m = build_from_fixture(g, step).cuda().train()
        for j in range(2):
            loss, grads = _step(m, g, j, store, form)
            ops.raise_on_bad_indices()
            ref = float(g[p + f"b{j}.loss"])
            budget = 3e-5 * max(1.0, abs(ref)) + float(g[f"ref_err.{p}b{j}.loss"])
            print(form, "step", step, "batch", j, "loss", float(loss), ref, "err", abs(float(loss) - ref), "budget", budget)
            assert abs(float(loss) - ref) <= budget
            for k in names:
                want = torch.from_numpy(g[p + f"b{j}.grad." + k])
                err = float((grads[my_name(k)].cpu() - want).abs().max())
                budget = 5e-6 + 5e-4 * float(want.abs().max()) + float(g[f"ref_err.{p}b{j}.grad." + k])
                print(form, "step", step, "batch", j, "grad", k, err, "budget", budget)
                assert err <= budget, (k, err)
            assert len(names) == len(grads) == 27
        m.eval()
        feat = m.compute_item(store)
        err = float((feat.cpu() - torch.from_numpy(g["eval.item_feature"])).abs().max())
        print("item features", err, "budget", 3e-5 + float(g["ref_err.item_feature"]))
        assert err <= 3e-5 + float(g["ref_err.item_feature"])
        scores = m.predict(win, feat)
        err = float((scores.cpu() - torch.from_numpy(g[p + "eval.scores"])).abs().max())
        print("step", step, "scores", err, "budget", 1e-4 + float(g[f"ref_err.{p}scores"]))
        assert tuple(scores.shape) == (len(win), feat.shape[0]) and err <= 1e-4 + float(g[f"ref_err.{p}scores"])
        # the Trainer's generic fused path: encode_last -> ops.score_topk, against predict + the two masks + topk
        K, Bw = 5, len(win)
        hist = [sorted(set(w[w != 0].tolist())) for w in g["eval.windows"]]
        hu = torch.tensor([b for b in range(Bw) for _ in hist[b]], dtype=torch.int64)
        hi = torch.tensor([i for b in range(Bw) for i in hist[b]], dtype=torch.int64)
        ptr, items = ops.history_csr(hu, hi, Bw, "cuda")
        out, last = m.encode_last(win, feat)
        assert tuple(out.shape) == (Bw, 1, feat.shape[1])
        idx, _ = ops.score_topk(last, last.stride(0), Bw, feat, K, ptr, items)
        ops.raise_on_bad_indices()
        masked = scores.clone()
        masked[:, 0] = -np.inf
        masked[(hu.cuda(), hi.cuda())] = -np.inf
        assert torch.equal(idx, torch.topk(masked, K, dim=-1).indices)


# ------------------------------------------------------------------------------------------------------------ 5. determinism, errors
def test_two_fresh_models_give_the_same_bits(gold):
    store = torch.from_numpy(gold["store"].astype(np.float32)).cuda()
    assert_two_fresh_models_agree(lambda: build_from_fixture(gold, 2).cuda().train(), lambda m, j: _step(m, gold, j, store, "positions"),
                                  28)


def test_bad_position_raises_index_error():
    B, L, D, M, step = SHAPES[0]
    m, seq, tgt, E = _case(B, L, D, M, step)
    E = E.requires_grad_(True)
    ops.raise_on_bad_indices()
    for where, val in (("node", M), ("target", M), ("target", -2), ("node", -1)):
        s2, t2 = seq.copy(), tgt.copy()
        if where == "node":
            s2[0, 0] = val
        else:
            t2[0, 1] = val
        m.loss_from_embeddings(E, torch.from_numpy(s2).cuda(), torch.from_numpy(t2).cuda()).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m.loss_from_embeddings(E, torch.from_numpy(seq).cuda(), torch.from_numpy(tgt).cuda()).backward()
    ops.raise_on_bad_indices()                                      # a clean batch leaves the word clear
    with pytest.raises(ValueError):
        m.loss_from_embeddings(E, torch.from_numpy(seq[:, :L - 1]).cuda(), torch.from_numpy(tgt).cuda())


# ------------------------------------------------------------------------------------------------------------ 6. optimizer
def test_optimizer_steps_both_groups_and_its_state_round_trips(gold):
    """Four optim_args: the encoder group and a rec group without a table, [18, 19] parameters and 18 + 17 states; one step moves
    both and leaves gnn.linear_edge_f where it was; the torch-layout state loads into torch.optim.AdamW over the reference's two
    groups and back."""
    store = torch.from_numpy(gold["store"].astype(np.float32)).cuda()

    def moved(moved, trainable):
        assert moved <= trainable and set(R.NAMES) <= moved and not set(R.EDGE_F) & moved
        assert sum("visual_encoder" in k for k in moved) >= 15     # (a key projection's bias has a zero gradient: it may stay)

    with_state = [i for i in range(37) if i not in (18 + 10, 18 + 11)]                      # linear_edge_f: no state
    assert_optimizer_state_round_trips(lambda: build_from_fixture(gold, 2, tune=37).cuda().train(),
                                       lambda m: _step(m, gold, 0, store, "positions"), [18, 19], with_state, moved=moved)


# ------------------------------------------------------------------------------------------------------------ 7. end to end
def test_main_py_trains_evaluates_and_the_checkpoint_reloads(tmp_path):
    """main.py on TinyInter with synthetic 64 x 64 images and the tiny tower, two epochs, through the fused evaluation: finite losses
    that change, Recall@10 and NDCG@10 reported from the reloaded checkpoint, whose state_dict loads with strict=True."""
    from pixelrec_amd.utils import get_model

    _, _, ck, config, data = run_main_py(tmp_path, "model: MOSRGNN\nembedding_size: 32\nstep: 2\n")
    rec = [k for k in ck["state_dict"] if not k.startswith("visual_encoder.")]
    assert list(ck["state_dict"])[-19:] == rec and [k for k in rec if k not in R.EDGE_F] == R.NAMES
    assert [len(x["params"]) for x in ck["optimizer"]["param_groups"]] == [18, 19]        # the reference's two groups
    fresh = get_model("MOSRGNN")(config, data)
    fresh.load_state_dict(ck["state_dict"], strict=True)
