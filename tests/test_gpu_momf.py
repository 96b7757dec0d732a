"""MOMF on the gfx950 kernels: the two-sink gradient kernel (pxr_momf_pair_grad_f32) against MF's sparse sink bit for bit, the head's
shift argument (pxr_mf_pair_fwd_eps_f32), the head without the encoder against the float64 restatement, the model against the
fixture of the reference's own MOMF in both configurations and both input forms (loss, every gradient, the BatchNorm running
statistics, compute_item, predict), the batch-wide dedup against one row per position, the lazy user table against a dense sweep,
the optimizer's two groups with the table in the second, bad ids, and main.py end to end.  Every test here needs the new entries,
the new ops or the new class, so each fails without the feature."""
import os

import numpy as np
import pytest
import torch

from pixelrec_amd import lib as _l
from pixelrec_amd import ops
from tests import momf_restate as R
from tests.mo_common import (FOUR, GOLD, LRS, assert_two_fresh_models_agree, bits as _bits, my_name, run_main_py, trainer_optimizer)
from tests.test_momf_cpu import CONFIGS, _config, build_from_fixture

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ 1. the two sinks
def _pair_case(B, D, U, M, seed, cross=False):
    """user [B] in [0, U), index [B, 2] positions in [0, M - 1) -- row M - 1 is read by nobody --, no sample whose two positions are
    equal; repeats come from the small ranges.  cross: position M - 2 sits at occurrences 3 and 130 of index.view(-1) and nowhere
    else, user U - 1 at samples 1 and 66 and nowhere else (a segment that leaves the 64-wide ballot window, in both sinks)."""
    rng = np.random.default_rng(seed)
    hi_u, hi_m = (U - 1, M - 2) if cross else (U, M - 1)
    user = rng.integers(0, hi_u, size=B)
    index = rng.integers(0, hi_m, size=(B, 2))
    index[:, 1] = np.where(index[:, 1] == index[:, 0], (index[:, 0] + 1) % hi_m, index[:, 1])
    if cross:
        flat = index.reshape(-1)
        flat[3] = flat[130] = M - 2
        user[1] = user[66] = U - 1
    assert (index[:, 0] != index[:, 1]).all()
    return torch.from_numpy(user).cuda(), torch.from_numpy(index).cuda()


@pytest.mark.parametrize("B,D,U,M,cross", [(6, 8, 5, 7, False), (9, 260, 5, 8, False), (5, 4096, 4, 7, False), (70, 64, 40, 60, True),
                                           (1, 8, 3, 4, False)])
def test_grad_kernel_is_mfs_table_gradient_in_two_sinks(B, D, U, M, cross):
    """One MF-layout table [spare | user rows | E rows] with MF's rows[3B] through pxr_mf_table_grad_f32, and the split operands
    through pxr_momf_pair_grad_f32, in the head's mode (scaled by grad_scale and the device scale) and in occ mode: the user slots
    carry the same ids and row bits, every item slot's sum sits in dE at its position bit for bit, and every row of dE nobody reads
    is +0.0 although the block held NaN before the call.  D = 8: a row shorter than a wave; 260: a partial second chunk (CH = 2);
    4096 with B = 5: CH = 16 and a last block with one live wave of four; B = 70: segments across the ballot window; B = 1."""
    user, index = _pair_case(B, D, U, M, 100 * B + D, cross)
    g = torch.Generator().manual_seed(B + D)
    utable = (torch.randn(1 + U, D, generator=g) * 0.3).cuda()
    E = (torch.randn(M, D, generator=g) * 0.3).cuda()
    table = torch.cat((utable, E)).contiguous()
    occ = torch.randn(3 * B, D, generator=g).cuda()
    mf_rows = ops.mf_pair_rows(user, index, U, M)
    rows = ops.momf_pair_rows(user, index, U, M)
    ops.raise_on_bad_indices()
    assert torch.equal(rows[:B], mf_rows[:B]) and torch.equal(rows[B:], index.view(-1)) and torch.equal(mf_rows[B:], 1 + U + rows[B:])
    if cross:
        flat = rows[B:].tolist()
        assert [k for k, v in enumerate(flat) if v == M - 2] == [3, 130] and [b for b, v in enumerate(user.tolist()) if v == U - 1] == [1, 66]
    loss_mf, coef_mf = ops.mf_pair_fwd(table, table, B, rows=mf_rows)
    loss, coef = ops.mf_pair_fwd(utable, E, B, rows=rows)              # two base pointers, one row list: the same head
    assert torch.equal(_bits(coef), _bits(coef_mf)) and torch.equal(_bits(loss), _bits(loss_mf))
    gs = torch.tensor([0.75], device="cuda")
    read = torch.zeros(M, dtype=torch.bool, device="cuda")
    read[rows[B:]] = True
    assert not bool(read[M - 1])
    for mode in ("head", "occ"):
        kw_mf = dict(table=table, coef=coef, grad_scale=2.0, grad_scale_dev=gs) if mode == "head" else dict(occ=occ)
        kw = dict(utable=utable, E=E, coef=coef, grad_scale=2.0, grad_scale_dev=gs) if mode == "head" else dict(occ=occ)
        sp_mf = ops.SparseRows(3 * B, D, "cuda")
        sp_mf.rows.fill_(float("nan"))
        ops.mf_table_grad(mf_rows, B, sp_mf, **kw_mf)
        outs = []
        for _ in range(2):
            sp = ops.SparseRows(B, D, "cuda")
            sp.rows.fill_(float("nan"))
            dE = torch.full((M, D), float("nan"), device="cuda")
            got = ops.momf_pair_grad(rows, B, sp, M, out=dE, **kw)
            assert got.data_ptr() == dE.data_ptr() and sp.count() == B
            outs.append((sp.idx.clone(), sp.rows.clone(), dE))
        (idx, srows, dE), (idx2, srows2, dE2) = outs
        assert torch.equal(idx, idx2) and torch.equal(_bits(srows), _bits(srows2)) and torch.equal(_bits(dE), _bits(dE2))
        assert torch.equal(idx, sp_mf.idx[:B]) and torch.equal(_bits(srows), _bits(sp_mf.rows[:B])), mode          # the user sink
        live = sp_mf.idx[B:] > 0
        pos = sp_mf.idx[B:][live] - (1 + U)
        assert sorted(pos.tolist()) == torch.nonzero(read).view(-1).tolist()            # one live item slot per position read
        assert torch.equal(_bits(dE[pos]), _bits(sp_mf.rows[B:][live])), mode           # the item sink: the same sums, dense
        assert int(_bits(dE[~read]).abs().max()) == 0                                   # +0.0 where a NaN stood before the call
        assert bool(torch.isfinite(dE).all()) and float(dE[read].abs().max()) > 0


def test_grad_kernel_refuses_what_it_cannot_serve():
    from pixelrec_amd.lib import PxrError

    user, index = _pair_case(4, 8, 5, 7, 1)
    rows = ops.momf_pair_rows(user, index, 5, 7)
    utable, E, coef = torch.zeros(6, 8, device="cuda"), torch.zeros(7, 8, device="cuda"), torch.zeros(4, device="cuda")
    sp = ops.SparseRows(4, 8, "cuda")
    ops.momf_pair_grad(rows, 4, sp, 7, utable=utable, E=E, coef=coef)
    with pytest.raises(PxrError):
        ops.momf_pair_grad(rows, 4, ops.SparseRows(3, 8, "cuda"), 7, utable=utable, E=E, coef=coef)      # too few sparse slots
    with pytest.raises(PxrError):
        ops.momf_pair_grad(rows, 4, sp, 7, utable=utable, E=E, coef=coef, out=E)                         # dE must not alias E
    with pytest.raises(PxrError):
        ops.momf_pair_grad(rows, 4, sp, 7, occ=torch.zeros(11, 8, device="cuda"))                        # occ is [3B, D]
    with pytest.raises(PxrError):
        ops.momf_pair_grad(rows[:11], 4, sp, 7, utable=utable, E=E, coef=coef)                           # rows is [3B]


# ------------------------------------------------------------------------------------------------------------ 2. the head's eps
def test_eps_is_an_argument():
    """eps = 1e-8 is pxr_mf_pair_fwd_f32 (the entry MF has called so far, reached here through ctypes) bit for bit; eps = 0 leaves
    the coef bits and gives lossrow = -log sigmoid(x), against float64 within 4 ulp of the value (and a float32 denormal's worth
    where it underflows), at x = 0, +-1.5, +-30, +-100, +-200 and +-1e4 -- exact in float32 by construction -- with every value
    finite (the reference's log(sigmoid(-1e4)) is -inf in float32)."""
    xs = [0.0, 1.5, -1.5, 30.0, -30.0, 88.5, 100.0, -100.0, 200.0, -200.0, 1e4, -1e4]
    B, H = len(xs), 8
    u = torch.zeros(B, H)
    u[:, 2] = torch.tensor(xs)
    it = torch.zeros(2 * B, H)
    it[0::2, 2] = 1.0                                               # x_b = <u_b, i+_b> - <u_b, i-_b> = xs[b], exactly
    u, it = u.cuda(), it.cuda()
    old = torch.full((2 * B + 1,), float("nan"), device="cuda")
    _l.check(_l.load().pxr_mf_pair_fwd_f32(_l.ptr(u), _l.ptr(it), None, H, B, _l.ptr(old[:B]), _l.ptr(old[B:2 * B]), _l.ptr(old[2 * B:]),
                                           _l.stream_ptr()), "pxr_mf_pair_fwd_f32")
    new = torch.full((2 * B + 1,), float("nan"), device="cuda")
    ops.mf_pair_fwd(u, it, B, out=new, eps=1e-8)
    dflt = torch.full((2 * B + 1,), float("nan"), device="cuda")
    ops.mf_pair_fwd(u, it, B, out=dflt)
    assert torch.equal(_bits(new), _bits(old)) and torch.equal(_bits(dflt), _bits(old))
    zero = torch.full((2 * B + 1,), float("nan"), device="cuda")
    loss, coef = ops.mf_pair_fwd(u, it, B, out=zero, eps=0.0)
    assert torch.equal(_bits(coef), _bits(old[:B])) and bool(torch.isfinite(zero).all()) and bool(torch.isfinite(old).all())
    x64 = torch.tensor(xs, dtype=torch.float64)
    want = -torch.nn.functional.logsigmoid(x64)
    got = zero[B:2 * B].cpu().double()
    err, tol = (got - want).abs(), 4 * U32 * want.abs() + 2e-38
    print("lossrow", got.tolist(), "float64", want.tolist(), "err", err.tolist())
    assert bool((err <= tol).all())
    assert float(got[-1]) == 1e4 and float(got[-3]) == 200.0         # where log(sigmoid(x)) in float32 is -inf
    assert abs(float(loss) - float(want.mean())) <= (B + 8) * U32 * float(want.mean())
    c64 = -torch.sigmoid(-x64) / B
    assert bool(((coef.cpu().double() - c64).abs() <= 4 * U32 * c64.abs() + 2e-38).all())
    shifted = old[B:2 * B].cpu().double()
    assert bool(((shifted - (want - 1e-8)).abs() <= 4 * U32 * want.abs() + 2e-8 * U32 + 2e-38).all())


# ------------------------------------------------------------------------------------------------------------ 3. the head alone
class _DL:
    user_num, item_num = 11, 13


def _tiny_model(D, hidden=(), seed=0):
    import pixelrec_amd.model as M

    torch.manual_seed(seed)
    m = M.MOMF(_config(D, 37, hidden), _DL())
    with torch.no_grad():                                           # biases and BatchNorm weights off their init, so that their
        for mlp in (m.user_mlp_layers, m.item_mlp_layers):         # part in the function shows
            for p in mlp.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))
    return m.cuda().train()


def _rec(m, dtype):
    L = len(m.mlp_hidden_size)
    sd = m.state_dict()
    return {k: (sd[k].detach().to(dtype) if sd[k].is_floating_point() else sd[k].clone()) for k in R.state_names(L)}


def _head_case(D, hidden, B=16, M=20):
    m = _tiny_model(D, hidden)
    user, index = _pair_case(B, D, _DL.user_num, M, 7 * B + D)
    E = (torch.randn(M, D, generator=torch.Generator().manual_seed(D + B)) * 0.5).cuda()
    L = len(hidden)
    res = {dt: R.loss_and_grads(_rec(m, dt), L, E.to(dt), user, index) for dt in (torch.float64, torch.float32)}
    return m, user, index, E, res


def _user_rows(m):
    """The sparse user rows of the last backward as the dense gradient of user_embedding.weight."""
    return m.sparse_table_grad.to_dense(1 + m.user_num)[1:]


def _head_grads(m, E):
    L = len(m.mlp_hidden_size)
    got = {k: m.get_parameter(k).grad.detach().clone() for k in R.trainable(R.tower_names(L))}
    got[R.TABLE] = _user_rows(m)
    got[R.E_KEY] = E.grad.detach().clone()
    return got


def _assert_grads(tag, got, res):
    (_, g64, _), (_, g32, _) = res[torch.float64], res[torch.float32]
    assert set(got) == set(g64)
    for k in got:
        err, d32 = float((got[k].double() - g64[k]).abs().max()), float((g32[k].double() - g64[k]).abs().max())
        big = float(g64[k].abs().max())
        print(tag, "grad", k, "err", err, "float32 restatement", d32, "largest entry", big)
        assert err <= 2 * d32 + 1e-6 * big, k


@pytest.mark.parametrize("D,hidden", [(64, ()), (512, ()), (64, (12, 8)), (512, (12, 8))])
def test_head_without_the_encoder_matches_float64(D, hidden):
    """loss_from_embeddings on a random leaf E against momf_restate in float64 on the same device, by tests/test_gpu_modin.py's
    rule: the loss within 2 |L32 - L64| + 2e-6 max(1, |L64|), every gradient (the tower tensors, dE and the scattered sparse user
    rows) within 2 d32 + 1e-6 max|g64|, L32 / d32 from the float32 restatement on the same inputs.  Rows of E nobody reads get
    exactly zero and only the batch's users have a row; the no_grad call gives the same loss bits; a detached E still drives the
    backward and leaves the user rows."""
    m, user, index, E, res = _head_case(D, hidden)
    E = E.requires_grad_(True)
    (L64, _, _), (L32, _, _) = res[torch.float64], res[torch.float32]
    loss = m.loss_from_embeddings(E, user, index)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    ops.raise_on_bad_indices()
    print("loss", float(loss.detach()), L64, "float32 restatement", L32)
    assert abs(float(loss.detach()) - L64) <= 2 * abs(L32 - L64) + 2e-6 * max(1.0, abs(L64))
    assert E.grad.shape == E.shape
    got = _head_grads(m, E)
    _assert_grads((D, hidden), got, res)
    for k in got:                                                   # a Linear bias in front of a BatchNorm: exactly zero, not noise
        if "_mlp_layers." in k and k.endswith(".bias") and int(k.split(".")[2]) % 4 == 1:
            assert int(_bits(got[k]).abs().max()) == 0, k
    read = torch.zeros(E.shape[0], dtype=torch.bool, device="cuda")
    read[index.view(-1)] = True
    assert not bool(read[-1]) and int(_bits(E.grad[~read]).abs().max()) == 0 and float(E.grad[read].abs().max()) > 0
    sp = m.sparse_table_grad
    assert sp.count() == user.numel() and sorted(sp.idx[sp.idx > 0].tolist()) == sorted(set((1 + user).tolist()))
    with torch.no_grad():
        again = m.loss_from_embeddings(E.detach(), user, index)
    assert not again.requires_grad and torch.equal(_bits(again), _bits(loss.detach()))
    rows_before = got[R.TABLE]
    m.sparse_table_grad = None
    frozen = m.loss_from_embeddings(E.detach(), user, index)
    assert frozen.requires_grad
    frozen.backward()
    assert torch.equal(_bits(_user_rows(m)), _bits(rows_before))    # the same step again: the same user rows
    for k in R.trainable(R.tower_names(len(hidden))):
        assert torch.equal(_bits(m.get_parameter(k).grad), _bits(got[k])), k


def test_bad_position_and_bad_user_raise_index_error_and_one_row_towers_value_error():
    m = _tiny_model(8)
    E = torch.randn(9, 8).cuda().requires_grad_(True)
    user, index = _pair_case(4, 8, _DL.user_num, 9, 1)
    ops.raise_on_bad_indices()
    for where, val in (("p", 9), ("p", -2), ("u", _DL.user_num), ("u", -1)):
        u2, i2 = user.clone(), index.clone()
        if where == "p":
            i2[0, 1] = val
        else:
            u2[2] = val
        m.loss_from_embeddings(E, u2, i2).backward()
        with pytest.raises(IndexError):
            ops.raise_on_bad_indices()
    m.loss_from_embeddings(E, user, index).backward()
    ops.raise_on_bad_indices()                                      # a clean batch leaves the word clear
    mt = _tiny_model(8, (12, 8))
    with pytest.raises(ValueError):
        mt.loss_from_embeddings(E, user[:1], index[:1])
    with pytest.raises(ValueError):
        m.loss_from_embeddings(E, user, index[:, :1])


# ------------------------------------------------------------------------------------------------------------ 5. the dedup
@pytest.mark.parametrize("D,hidden", [(64, ()), (64, (12, 8))])
def test_dedup_does_not_change_the_function(D, hidden):
    """One row per position (the reference's form: E_x[2b + t] = E[index_{b,t}], positions 2b + t) against the batch-wide dedup, by
    tests/test_gpu_modin.py::test_dedup_does_not_change_the_function's rule: the same loss bits; dE[r] is the sum of its copies'
    gradients, in float64 within (k + 1) 2^-24 sum|terms|; the same sparse user rows and tower gradients bit for bit -- they do not
    pass through the item sink -- and within the bounds of the float64 comparison."""
    m, user, index, E, res = _head_case(D, hidden)
    E = E.requires_grad_(True)
    loss = m.loss_from_embeddings(E, user, index)
    loss.backward()
    got = _head_grads(m, E)
    flat = index.view(-1)
    Ex = E.detach()[flat].clone().requires_grad_(True)
    pos = torch.arange(flat.numel(), device="cuda").view(index.shape)
    loss_x = m.loss_from_embeddings(Ex, user, pos)
    loss_x.backward()
    ops.raise_on_bad_indices()
    assert torch.equal(_bits(loss_x.detach()), _bits(loss.detach()))
    terms = Ex.grad.double()
    M = E.shape[0]
    z = lambda: torch.zeros(M, D, dtype=torch.float64, device="cuda")
    d64, dabs = z().index_add_(0, flat, terms), z().index_add_(0, flat, terms.abs())
    k = torch.zeros(M, dtype=torch.float64, device="cuda").index_add_(0, flat, torch.ones_like(flat, dtype=torch.float64))
    over = (E.grad.double() - d64).abs() - (k[:, None] + 1) * U32 * dabs
    print("dE against the summed copies", float((E.grad.double() - d64).abs().max()), "most copies", int(k.max()))
    assert float(over.max()) <= 0 and int(k.max()) >= 2
    got_x = _head_grads(m, Ex)
    for name in got:
        if name != R.E_KEY:
            assert torch.equal(_bits(got_x[name]), _bits(got[name])), name
    got_x.pop(R.E_KEY)
    got.pop(R.E_KEY)
    for r in res.values():
        r[1].pop(R.E_KEY)
    _assert_grads("one row per position", got_x, res)


# ------------------------------------------------------------------------------------------------------------ 4. the fixture
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "momf_tiny.npz"))


def _inputs(g, j, store, form):
    user, item = torch.from_numpy(g[f"b{j}.user"]).cuda(), g[f"b{j}.item"]
    if form == "positions":                                         # what MoPairTrainBatcher.make_batch builds
        image_ids, index = np.unique(item, return_inverse=True)
        return user, torch.from_numpy(index.reshape(item.shape)).cuda(), store[torch.from_numpy(image_ids).cuda()]
    return user, store[torch.from_numpy(item).cuda()]               # momf.py:51: (user, item [B, 2, 3, H, W])


def _step(m, g, j, store, form):
    loss = m(_inputs(g, j, store, form))
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad and p.grad is not None and n != R.TABLE}
    grads[R.TABLE] = _user_rows(m)
    return loss.detach().clone(), grads


@pytest.mark.parametrize("form", ["positions", "reference"])
@pytest.mark.parametrize("c", CONFIGS)
def test_model_matches_the_reference_fixture(gold, c, form):
    """Loss, every gradient (the dense user table's from the sparse rows), the BatchNorm running statistics after each batch,
    compute_item and predict against the stored results of the reference's MOMF, identity towers and [12, 8], with the batch in the
    batcher's form and in the reference's 5-D form.  Budgets: the project's recorded ones for this tiny tower
    (tests/test_gpu_modin.py::test_model_matches_the_reference_fixture) -- loss 3e-5 max(1, |loss|), gradients 5e-6 + 5e-4 max|g|,
    item features (and the running statistics, which are feature statistics) 3e-5, scores 1e-4 -- each plus the quantity's stored
    ref_err."""
    g = gold
    m = build_from_fixture(g, c).cuda().train()
    store = torch.from_numpy(g["store"].astype(np.float32)).cuda()
    names = [str(k) for k in g[c + ".param.keys"]]
    stat_keys = [str(k) for k in g[c + ".stats.keys"]]
    for j in range(2):
        loss, grads = _step(m, g, j, store, form)
        ops.raise_on_bad_indices()
        ref = float(g[f"{c}.b{j}.loss"])
        budget = 3e-5 * max(1.0, abs(ref)) + float(g[f"ref_err.{c}.b{j}.loss"])
        print(c, form, "batch", j, "loss", float(loss), ref, "err", abs(float(loss) - ref), "budget", budget)
        assert abs(float(loss) - ref) <= budget
        for i, k in enumerate(names):
            want = torch.from_numpy(g[f"{c}.b{j}.grad." + k])
            err = float((grads[my_name(k)].cpu() - want).abs().max())
            budget = 5e-6 + 5e-4 * float(want.abs().max()) + float(g[f"ref_err.{c}.b{j}.grad"][i])
            print(c, form, "batch", j, "grad", k, err, "budget", budget)
            assert err <= budget, (k, err)
        assert len(names) == len(grads) == 8 * len(g[c + ".hidden"]) + 1 + 18
        sd = m.state_dict()
        for i, k in enumerate(stat_keys):
            want = torch.from_numpy(g[f"{c}.b{j}.stats." + k])
            if want.dtype == torch.int64:
                assert int(sd[k]) == int(want) == j + 1, k
                continue
            err = float((sd[k].cpu() - want).abs().max())
            print(c, form, "batch", j, "stats", k, err, "budget", 3e-5 + float(g[f"ref_err.{c}.b{j}.stats"][i]))
            assert err <= 3e-5 + float(g[f"ref_err.{c}.b{j}.stats"][i]), (k, err)
    m.eval()
    feat = m.compute_item(store)
    err = float((feat.cpu() - torch.from_numpy(g[c + ".eval.item_feature"])).abs().max())
    print(c, "item features", err, "budget", 3e-5 + float(g[f"ref_err.{c}.item_feature"]))
    assert err <= 3e-5 + float(g[f"ref_err.{c}.item_feature"])
    scores = m.predict(torch.from_numpy(g["eval.users"]).cuda(), feat)
    err = float((scores.cpu() - torch.from_numpy(g[c + ".eval.scores"])).abs().max())
    print(c, "scores", err, "budget", 1e-4 + float(g[f"ref_err.{c}.scores"]))
    assert tuple(scores.shape) == tuple(g[c + ".eval.scores"].shape) and err <= 1e-4 + float(g[f"ref_err.{c}.scores"])
    out, last = m.encode_last(torch.from_numpy(g["eval.users"]).cuda(), feat)
    assert tuple(out.shape) == (scores.shape[0], 1, m.out_size) and torch.equal(out[:, 0], last)


def test_both_input_forms_are_one_function_of_the_model(gold):
    """The same model and batch through the encoder in the batcher's form (each distinct image once) and in the reference's form
    (one image per position): identical loss bits (the tower is a per-image function, and the head reads the same rows), and every
    gradient within the fixture test's budgets of the other form's (the reference's own error left out)."""
    store = torch.from_numpy(gold["store"].astype(np.float32)).cuda()
    a, ga = _step(build_from_fixture(gold, "c1").cuda().train(), gold, 0, store, "positions")
    b, gb = _step(build_from_fixture(gold, "c1").cuda().train(), gold, 0, store, "reference")
    print("loss", float(a), float(b), "same bits", bool(torch.equal(_bits(a), _bits(b))))
    assert torch.equal(_bits(a), _bits(b))
    assert set(ga) == set(gb)
    for k in ga:
        err, big = float((ga[k] - gb[k]).abs().max()), float(ga[k].abs().max())
        assert err <= 5e-6 + 5e-4 * big, (k, err, big)


def test_two_fresh_models_give_the_same_bits(gold):
    store = torch.from_numpy(gold["store"].astype(np.float32)).cuda()
    assert_two_fresh_models_agree(lambda: build_from_fixture(gold, "c1").cuda().train(), lambda m, j: _step(m, gold, j, store, "positions"),
                                  1 + 35)


# ------------------------------------------------------------------------------------------------------------ 6. the lazy table
def _head_batches(n, B, U, M, D, seed):
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n):
        lo = 0 if s % 3 else U // 2                        # some rows sit out several steps, then come back
        user = torch.from_numpy(rng.integers(lo, lo + U // 2, size=B)).cuda()
        index = rng.integers(0, M, size=(B, 2))
        index[:, 1] = np.where(index[:, 1] == index[:, 0], (index[:, 0] + 1) % M, index[:, 1])
        E = torch.from_numpy(rng.standard_normal((M, D)).astype(np.float32) * 0.5).cuda()
        out.append((user, torch.from_numpy(index).cuda(), E))
    return out


def test_one_step_changes_only_the_batchs_user_rows():
    from pixelrec_amd.optim import PxrAdamW

    m = _tiny_model(64)
    opt = PxrAdamW(m, lr=1e-2, weight_decay=0.1)
    before = m.lazy_table().clone()
    (user, index, E), = _head_batches(1, 6, _DL.user_num, 9, 64, 3)
    opt.zero_grad()
    m.loss_from_embeddings(E, user, index).backward()
    opt.step()
    changed = torch.nonzero((m.lazy_table() != before).any(1)).view(-1).tolist()
    assert changed == sorted(set((1 + user).tolist())) and 0 not in changed        # nothing else has been swept yet
    m.sync_table()
    swept = torch.nonzero((m.lazy_table() != before).any(1)).view(-1).tolist()
    assert swept == list(range(1, 1 + _DL.user_num))                               # the decay reaches every row but the spare


@pytest.mark.parametrize("hidden", [(), (12, 8)])
def test_lazy_and_dense_table_updates_are_bit_identical(hidden, monkeypatch):
    """tests/test_gpu_mf.py::test_lazy_and_dense_table_updates_are_bit_identical on MOMF's head: twelve steps with rows that sit out
    and come back, sync_table(), under PXR_LAZY_REPLAY=exact -- the table, both moments and the flat buffer of the lazy schedule
    equal the dense sweep's bit for bit."""
    from pixelrec_amd.optim import PxrAdamW

    monkeypatch.setenv("PXR_LAZY_REPLAY", "exact")
    sd = {k: v.clone() for k, v in _tiny_model(64, hidden).state_dict().items()}
    batches = _head_batches(12, 16, _DL.user_num - 1, 24, 64, 4)
    res = {}
    for how in ("lazy", "dense"):
        m = _tiny_model(64, hidden, seed=1)
        m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        opt = PxrAdamW(m, lr=1e-2, weight_decay=0.1, table_update=how)
        for user, index, E in batches:
            opt.zero_grad()
            m.loss_from_embeddings(E, user, index).backward()
            opt.step()
        m.sync_table()
        opt.flush()
        torch.cuda.synchronize()
        res[how] = (m.lazy_table().clone(), opt._tm.clone(), opt._tv.clone(), m.flat_parameters()[0].clone())
    assert not torch.equal(res["lazy"][0][1:], sd[R.TABLE].cuda())
    for a, b in zip(res["lazy"], res["dense"]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 7. the optimizer
def test_optimizer_steps_both_groups_and_its_state_round_trips(gold):
    """mo_common.assert_optimizer_state_round_trips for a rec group WITH a table: four optim_args give the encoder group and the
    rec group, [18, 17] parameters; one step moves the encoder, the towers and the batch's user rows; the torch-layout state holds
    the table's moments as [user_num, D] and loads into torch.optim.AdamW over the reference's two groups and back."""
    from pixelrec_amd.optim import OptimizerGroup

    g, c = gold, "c1"
    store = torch.from_numpy(g["store"].astype(np.float32)).cuda()
    build = lambda: build_from_fixture(g, c).cuda().train()
    m = build()
    opt = trainer_optimizer(m, FOUR)
    assert isinstance(opt, OptimizerGroup)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt.zero_grad()
    _step(m, g, 0, store, "positions")
    opt.step()
    after = m.state_dict()
    moved = {k for k in before if not torch.equal(before[k], after[k])}
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    stats = {str(k) for k in g[c + ".stats.keys"]}
    assert moved <= trainable | stats and R.TABLE in moved and stats <= moved and any("visual_encoder" in k for k in moved)
    assert {k for k in R.trainable(R.tower_names(2)) if k.endswith("weight")} <= moved
    users = set(g["b0.user"].tolist())
    rows = torch.nonzero((before[R.TABLE] != after[R.TABLE]).any(1)).view(-1).tolist()
    assert set(rows) == set(range(int(g["meta"][0]))) and users < set(rows)      # state_dict() syncs the table: every row decayed
    sd = opt.state_dict(layout="torch")
    groups, with_state = [18, 17], list(range(35))
    assert [len(x["params"]) for x in sd["param_groups"]] == groups and sorted(sd["state"]) == with_state
    assert [(x["lr"], x["weight_decay"]) for x in sd["param_groups"]] == LRS
    enc = [p for n, p in m.named_parameters() if "visual_encoder" in n and p.requires_grad]
    recs = [m.get_parameter(k) for k in m.rec_parameter_names()]                 # the reference's registration order
    assert [tuple(sd["state"][18 + i]["exp_avg"].shape) for i in range(17)] == [tuple(p.shape) for p in recs]
    assert tuple(sd["state"][34]["exp_avg"].shape) == (int(g["meta"][0]), int(g["meta"][2]))         # the table: [user_num, D]
    tm = sd["state"][34]["exp_avg"]
    assert set(torch.nonzero(tm.abs().sum(1)).view(-1).tolist()) == users        # only the batch's users have a moment
    tor = torch.optim.AdamW([{"params": enc, "lr": 1.0, "weight_decay": 0.5}, {"params": recs, "lr": 2.0, "weight_decay": 0.25}])
    tor.load_state_dict(sd)                                                      # the layout the reference stores
    assert [(x["lr"], x["weight_decay"]) for x in tor.param_groups] == LRS
    opt2 = trainer_optimizer(build(), {**FOUR, "modal_lr": 5.0, "rec_lr": 7.0})
    opt2.load_state_dict(tor.state_dict())
    sd2 = opt2.state_dict(layout="torch")
    assert [x["params"] for x in sd2["param_groups"]] == [x["params"] for x in sd["param_groups"]]
    assert [(x["lr"], x["weight_decay"]) for x in sd2["param_groups"]] == LRS and sorted(sd2["state"]) == with_state
    for i in with_state:
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sd2["state"][i][key].cpu(), sd["state"][i][key].cpu()), (i, key)


# ------------------------------------------------------------------------------------------------------------ 8. end to end
def test_main_py_trains_evaluates_and_the_checkpoint_reloads(tmp_path):
    """main.py on TinyInter with synthetic 64 x 64 images and the tiny tower, two epochs, through the Trainer's generic pair
    evaluation, on the shipped identity towers (TinyInter's 761 pairs leave a one-row last batch at the helper's batch size of 8,
    which BatchNorm towers refuse as the reference's do): finite losses that change, Recall@10 and NDCG@10 reported from the
    reloaded checkpoint, whose state_dict has the reference's keys and loads with strict=True."""
    from pixelrec_amd.utils import get_model

    _, _, ck, config, data = run_main_py(tmp_path, "model: MOMF\nembedding_size: 32\ndropout_prob: 0\nmlp_hidden_size: []\n")
    keys = list(ck["state_dict"])
    assert keys[0] == R.TABLE and R.state_names(0) == [R.TABLE] and all(k.startswith("visual_encoder.") for k in keys[1:])
    assert [len(x["params"]) for x in ck["optimizer"]["param_groups"]] == [18, 1]          # the reference's two groups
    assert tuple(ck["state_dict"][R.TABLE].shape) == (data.user_num, 32)
    assert tuple(ck["optimizer"]["state"][18]["exp_avg"].shape) == (data.user_num, 32)     # the table's moments, reference-shaped
    fresh = get_model("MOMF")(config, data)
    fresh.load_state_dict(ck["state_dict"], strict=True)
