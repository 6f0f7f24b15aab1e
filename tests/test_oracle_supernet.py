"""Pins oracle/ref_supernet.py (the CPU restatement of search/model_search.py used by bench.py's cpu_baseline and by the
full-size supernet checks) to the fixtures oracle/make_golden.py generated from the unmodified reference."""
import numpy as np
import pytest
import torch

from oracle import ref_supernet
from oracle.seeded import seeded_input, seeded_state
from tests._util import assert_close_golden, golden_get, load_json, load_npz

WML = [4. / 12, 6. / 12, 8. / 12, 10. / 12, 1.]
CFG = dict(layers=6, Fch=12, width_mult_list=WML, prun_modes=['max', 'arch_ratio'], stem_head_width=[(1, 1), (8. / 12, 8. / 12)])


def _params(requires_grad=False):
    meta = load_json("supernet_meta.json")
    sd = seeded_state({k: torch.empty(v) for k, v in meta["state_shapes"].items()}, 777)
    for k in list(sd):
        if k.split("_")[0] in ("alpha", "beta", "ratio"):
            sd[k] = sd[k] * 5.0
    if requires_grad:
        for k, v in sd.items():
            if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
                v.requires_grad_(True)
    return sd


def test_oracle_supernet_eval_logits_match_reference():
    store = load_npz("supernet.npz")
    params = _params()
    x = seeded_input((2, 3, 128, 256), 31)
    for idx in (0, 1):
        with torch.no_grad():
            preds = ref_supernet.forward(params, CFG, x, idx, "max", training=False)
        for i, p in enumerate(preds):
            assert_close_golden(p[:, :, ::4, ::4], store, "eval_arch%d/pred%d_sub" % (idx, i), 2e-5, 1e-5, "arch%d pred%d" % (idx, i))


def test_oracle_supernet_losses_and_gradients_match_reference():
    store = load_npz("supernet.npz")
    x = seeded_input((2, 3, 128, 256), 31)
    target = torch.tensor(store["target"])
    for mode in ("pretrain", "search"):
        params = _params(requires_grad=True)
        np.random.seed(5)
        torch.manual_seed(6)
        loss = ref_supernet.loss(params, CFG, x, target, mode == "pretrain")
        loss.backward()
        want = float(store["%s_f32/loss" % mode][0])
        assert abs(float(loss.detach()) - want) <= 2e-5 * abs(want), (mode, float(loss.detach()), want)
        for key in store:
            if key.startswith("%s_f32/g/" % mode):
                pname = key[len("%s_f32/g/" % mode):].split("@")[0]
                want_g, step = golden_get(store, "%s_f32/g/%s" % (mode, pname))
                got = params[pname].grad.reshape(-1)[::step].numpy()
                denom = float(np.abs(want_g).max()) + 1e-12
                assert float(np.abs(got - want_g.reshape(-1)).max()) <= 2e-3 * denom, (mode, pname)


def test_oracle_supernet_l16_search_loss_matches_reference():
    """The oracle at the benchmarked depth and map size (F12.L16, 1x3x224x448: 7x14 maps zoomed to 3x7 through H//2) against the
    fixture the unmodified reference produced in fp64 - this is the checker bench.py's C3 / C5 parity gates and cpu_baseline use."""
    from fasterseg_amd import model_search
    store = load_npz("supernet_l16.npz")
    meta = load_json("supernet_l16_meta.json")
    cfg = dict(CFG, layers=16)
    net = model_search.Network_Multi_Path(19, 16, None, 12, WML, ['max', 'arch_ratio'], [(1, 1), (8. / 12, 8. / 12)])
    assert sum(p.numel() for p in net.parameters()) == meta["num_params"]
    sd = seeded_state(net.state_dict(), 778)
    del net
    params = {}
    for k, v in sd.items():
        if k.split("_")[0] in ("alpha", "beta", "ratio"):
            v = v * 5.0
        params[k] = v.double() if v.is_floating_point() else v
    x = seeded_input(tuple(meta["search"]["shape"]), 41).double()
    target = torch.tensor(store["search/target"])
    np.random.seed(5)
    torch.manual_seed(6)
    with torch.no_grad():
        loss = ref_supernet.loss(params, cfg, x, target, False)
    want = float(store["search/loss"][0])
    assert abs(float(loss) - want) <= 1e-6 * abs(want), (float(loss), want)


def _l16_params(dtype):
    from fasterseg_amd import model_search
    net = model_search.Network_Multi_Path(19, 16, None, 12, WML, ['max', 'arch_ratio'], [(1, 1), (8. / 12, 8. / 12)])
    sd = seeded_state(net.state_dict(), 778)
    del net
    params = {}
    for k, v in sd.items():
        if k.split("_")[0] in ("alpha", "beta", "ratio"):
            v = v * 5.0
        params[k] = v.to(dtype) if v.is_floating_point() else v
    return params


@pytest.mark.parametrize("mode", ["pretrain", "search"])
def test_oracle_supernet_l16_loss_matches_reference_at_benchmarked_batch(mode):
    """The oracle against the fixture of the benchmarked batches (tests/golden/supernet_l16_b*: pretrain 3 x 3x256x512, search
    2 x 3x224x448, distinct samples, the unmodified reference in fp64), in fp32: the `_loss` of the four passes."""
    store = load_npz("supernet_l16_b.npz")
    meta = load_json("supernet_l16_b_meta.json")
    shape = tuple(meta[mode]["shape"])
    assert shape == ((3, 3, 256, 512) if mode == "pretrain" else (2, 3, 224, 448))
    params = _l16_params(torch.float32)
    x = seeded_input(shape, 41)
    target = torch.tensor(store[mode + "/target"])
    assert not torch.equal(x[0], x[1]) and not torch.equal(target[0], target[1])
    np.random.seed(5)
    torch.manual_seed(6)
    with torch.no_grad():
        loss = ref_supernet.loss(params, dict(CFG, layers=16), x, target, mode == "pretrain")
    want = float(store[mode + "/loss"][0])
    assert abs(float(loss) - want) <= 2e-5 * abs(want), (float(loss), want)


def test_search_iteration_fixture_adam_steps_reproduce_the_stored_arch_params():
    """Internal consistency of tests/golden/search_iter_l16* (two iterations of train_search.py:225-250 by the unmodified reference,
    fp64): torch Adam(lr 3e-4, betas 0.5 / 0.999) fed the stored architecture gradients - a None gradient skips its tensor, as in the
    reference - reproduces the stored architecture parameters after each arch step, from the seeded start values."""
    store = load_npz("search_iter_l16.npz")
    meta = load_json("search_iter_l16_meta.json")
    names = meta["arch_params"]
    assert len(names) == 16 and sum(store["f64/it0/arch_param/" + k].size for k in names) == 822
    init = _l16_params(torch.float64)
    params = [torch.nn.Parameter(init[k].clone()) for k in names]
    opt = torch.optim.Adam(params, lr=3e-4, betas=(0.5, 0.999))
    for it in (0, 1):
        none = set(meta["it%d" % it]["arch_grad_none"])
        assert none == {k for k in names if "f64/it%d/arch_grad/%s" % (it, k) not in store}
        for k, p in zip(names, params):
            p.grad = None if k in none else torch.from_numpy(store["f64/it%d/arch_grad/%s" % (it, k)]).double()
        opt.step()
        for k, p in zip(names, params):
            want = store["f64/it%d/arch_param/%s" % (it, k)]
            assert np.abs(p.detach().numpy() - want).max() <= 1e-12, (it, k)
            if k in none:
                assert np.array_equal(want, init[k].numpy())
