"""Classifier-free guidance without a GPU: the bound of tests/cfg_bounds.py accepts an fp32 evaluation in the kernels' order and
rejects every mutant, ClassifierFreeGuidedModel on host tensors is two model calls combined by hand (both layouts of the stacked
batch; the two-person rows keep their partner), caption dropout of both trainers, and set_sampler's guidance_scale."""
import types

import pytest
import torch

import cfg_bounds as cb
import hig_amd
from hig_amd.models import gaussian_diffusion as gdm
from hig_amd.models.guidance import split_rows, stack_rows

N = 1000


# ---- 1. the bound has teeth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,group", cb.BG)
@pytest.mark.parametrize("per", cb.PER_SAMPLE)
def test_fp32_evaluation_is_inside_the_bounds(per, B, group):
    for kind in ("ddim", "p"):
        x2, eps2, z, t2, tab = cb.cfg_case(B, group, per, kind, seed=per + B)
        for s in cb.SCALES:
            eg, e_g = cb.combine_bound(eps2, s, B, group)
            assert cb.ratio(cb.combine_eval(eps2, s, B, group, dtype=cb.F32), eg, e_g) <= 1.0, (s,)
            if kind == "p":
                (xp, b), (x0, b0) = cb.p_bound(x2, eps2, z, t2, tab, s, B, group)
                o, o0 = cb.p_eval(x2, eps2, z, t2, tab, s, B, group, dtype=cb.F32)
                assert torch.isfinite(b).all() and cb.ratio(o, xp, b) <= 1.0 and cb.ratio(o0, x0, b0) <= 1.0, (s,)
                continue
            for eta in cb.ETAS:
                for clip in cb.CLIPS:
                    zz = None if eta == 0 else z
                    (xp, b), (x0, b0) = cb.ddim_bound(x2, eps2, zz, t2, tab, s, B, group, eta, clip)
                    assert torch.isfinite(xp).all() and torch.isfinite(b).all() and (b >= 0).all()
                    o, o0 = cb.ddim_eval(x2, eps2, zz, t2, tab, s, B, group, eta, clip, dtype=cb.F32)
                    assert cb.ratio(o, xp, b) <= 1.0 and cb.ratio(o0, x0, b0) <= 1.0, (s, eta, clip)


@pytest.mark.parametrize("mutant", cb.MUTANTS)
def test_bounds_reject_mutant(mutant):
    """On every case of the input set where the mutant computes something else (cfg_bounds.visible), and on at least one.  Under
    the clamp an element whose x0 leaves [-1, 1] on the same side in the truth and in the mutant shows nothing, and a case of ONE
    element can consist of such an element: the clamped DDIM cases are asserted for per_sample > 1."""
    seen = 0
    unequal = mutant == "state_from_uncond_row"
    for per in cb.PER_SAMPLE:
        for B, group in cb.BG:
            xd, ed, z, td, tabd = cb.cfg_case(B, group, per, "ddim", seed=per + B, unequal=unequal)
            xq, eq, zq, tq, tabq = cb.cfg_case(B, group, per, "p", seed=per + B, unequal=unequal)
            for s in cb.SCALES:
                if mutant != "combine_after_clamp" and mutant != "state_from_uncond_row" and cb.visible(mutant, s, group, B, 0, unequal):
                    eg, e_g = cb.combine_bound(ed, s, B, group)
                    assert cb.ratio(cb.combine_eval(ed, s, B, group, mutant=mutant), eg, e_g) > 1.0, (mutant, per, B, group, s)
                if cb.visible(mutant, s, group, B, 0, unequal, kind="p"):
                    (xp, b), _ = cb.p_bound(xq, eq, zq, tq, tabq, s, B, group)
                    out = cb.p_eval(xq, eq, zq, tq, tabq, s, B, group, mutant=mutant)[0]
                    assert cb.ratio(out, xp, b) > 1.0, (mutant, "p", per, B, group, s)
                    seen += 1
                for eta in cb.ETAS:
                    for clip in cb.CLIPS:
                        if not cb.visible(mutant, s, group, B, clip, unequal) or (clip and per == 1):
                            continue
                        zz = None if eta == 0 else z
                        (xp, b), _ = cb.ddim_bound(xd, ed, zz, td, tabd, s, B, group, eta, clip)
                        out = cb.ddim_eval(xd, ed, zz, td, tabd, s, B, group, eta, clip, mutant=mutant)[0]
                        assert cb.ratio(out, xp, b) > 1.0, (mutant, per, B, group, s, eta, clip)
                        seen += 1
    assert seen > 0


def test_equal_branches_give_the_unguided_step():
    """eps_u == eps_c: d = 0, eps_g = eps_u exactly, in fp32 too -- the guided evaluation is the unguided one, bit for bit."""
    x2, eps2, z, t2, tab = cb.cfg_case(4, 2, 5, "ddim", seed=1)
    rc, ru = cb.rows(4, 2)
    eps2[ru] = eps2[rc]
    for s in cb.SCALES:
        assert torch.equal(cb.combine_eval(eps2, s, 4, 2, dtype=cb.F32), eps2[rc])
        o = cb.ddim_eval(x2, eps2, z, t2, tab, s, 4, 2, 0.5, 1, dtype=cb.F32)
        want = cb.db.ddim_eval(x2[rc], eps2[rc], z, t2[rc], tab, 0.5, 1, dtype=cb.F32)
        assert torch.equal(o[0], want[0]) and torch.equal(o[1], want[1])


def test_layout_helpers_agree_with_the_header_formula():
    for B, group in cb.BG + ((8, 4), (8, 1)):
        v = torch.arange(B * 3, dtype=torch.float32).view(B, 3)
        got = stack_rows(v, v + 100, group)
        assert torch.equal(got, cb.stack(v, v + 100, group))
        c, u = split_rows(got, group)
        assert torch.equal(c, v) and torch.equal(u, v + 100)
        caps = ["c%d" % i for i in range(B)]
        rc, ru = cb.rows(B, group)
        st = stack_rows(caps, [""] * B, group)
        assert [st[i] for i in rc.tolist()] == caps and all(st[i] == "" for i in ru.tolist())


# ---- 2. the wrapper on host tensors -----------------------------------------------------------------------------------------
class PairStub:
    """A model whose row i also sees row i + half (mod the batch), as the interaction attention pairs them, and its own text
    and length rows."""

    def __init__(self):
        self.calls = []

    def parameters(self):
        return iter([torch.zeros(1)])

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def __call__(self, x, t, xf_proj=None, xf_out=None, length=None, text=None):
        self.calls.append(x.shape[0])
        half = x.shape[0] // 2
        partner = torch.roll(x, half, 0)
        tx = xf_proj[:, :1, None] + xf_out.sum(dim=(1, 2))[:, None, None]
        if text is not None:
            tx = tx + torch.tensor([float(len(c)) for c in text])[:, None, None]
        return x * 0.5 + partner * 0.25 + tx + t.float()[:, None, None] * 0.01 + length.float()[:, None, None] * 0.1


def wrapper_case(B):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 4, 6, generator=g)
    t = torch.randint(0, 50, (B,), generator=g)
    kw = dict(xf_proj=torch.randn(B, 8, generator=g), xf_out=torch.randn(B, 3, 8, generator=g),
              length=torch.arange(B) + 1)
    un = dict(xf_proj=torch.randn(1, 8, generator=g), xf_out=torch.randn(1, 3, 8, generator=g))
    return x, t, kw, un


@pytest.mark.parametrize("s", (0.0, 1.0, 2.5, -1.0))
def test_wrapper_is_two_calls_combined_by_hand_single_person_layout(s):
    B = 6
    x, t, kw, un = wrapper_case(B)
    m = PairStub()
    g = hig_amd.ClassifierFreeGuidedModel(m, s, un)
    out = g(x, t, **kw)
    assert m.calls == [2 * B]                                       # one call at 2 B
    # group = B: [cond; uncond], so in the stacked call a row's partner is its OWN other branch...
    x2 = torch.cat([x, x])
    both = m(x2, torch.cat([t, t]), xf_proj=torch.cat([kw["xf_proj"], un["xf_proj"].expand(B, -1)]),
             xf_out=torch.cat([kw["xf_out"], un["xf_out"].expand(B, -1, -1)]), length=torch.cat([kw["length"]] * 2))
    c, u = both[:B], both[B:]
    assert torch.equal(out, u + (c - u) * s)
    assert next(g.parameters()) is not None and g.eval() is g and g.train() is g


@pytest.mark.parametrize("s", (0.0, 1.0, 2.5))
def test_wrapper_two_person_layout_keeps_the_partner(s):
    """group = pairs: each branch is a model batch [p1; p2] of its own, so the stacked call equals TWO separate calls."""
    P = 3
    B = 2 * P
    x, t, kw, un = wrapper_case(B)
    m = PairStub()
    out = hig_amd.ClassifierFreeGuidedModel(m, s, un, group=P)(x, t, **kw)
    assert m.calls == [2 * B]
    c = m(x, t, **kw)
    u = m(x, t, xf_proj=un["xf_proj"].expand(B, -1), xf_out=un["xf_out"].expand(B, -1, -1), length=kw["length"])
    assert torch.equal(out, u + (c - u) * s)
    # and with group = B the stacked batch pairs a row with its own other branch instead: not the two-person model's pairing
    wrong = hig_amd.ClassifierFreeGuidedModel(m, s, un, group=B)(x, t, **kw)
    assert not torch.equal(wrong, out)


def test_wrapper_stacks_captions_and_validates():
    B = 4
    x, t, kw, _ = wrapper_case(B)
    m = PairStub()
    caps = ["a person waves", "two people hug", "a person jumps", "a person sits down"]
    g = hig_amd.ClassifierFreeGuidedModel(m, 2.0, dict(text=[""]), group=2)
    out = g(x, t, text=caps, **kw)
    st = stack_rows(caps, [""] * B, 2)
    assert st == caps[:2] + ["", ""] + caps[2:] + ["", ""]
    both = m(stack_rows(x, x, 2), stack_rows(t, t, 2), text=st, **{k: stack_rows(v, v, 2) for k, v in kw.items()})
    c, u = split_rows(both, 2)
    assert torch.equal(out, u + (c - u) * 2.0)
    for bad in (float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            hig_amd.ClassifierFreeGuidedModel(m, bad, dict(text=[""]))
    with pytest.raises(ValueError):
        hig_amd.ClassifierFreeGuidedModel(m, 2.0, {})
    with pytest.raises(ValueError):
        hig_amd.ClassifierFreeGuidedModel(m, 2.0, dict(text=[""]), group=3)(x, t, text=caps, **kw)


def test_wrapper_runs_through_every_sampler_entry_on_host_tensors():
    B = 4
    x, t, kw, un = wrapper_case(B)
    m = PairStub()
    g = hig_amd.ClassifierFreeGuidedModel(m, 2.5, un)
    gd = hig_amd.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", 50), model_mean_type=gdm.ModelMeanType.EPSILON,
                                   model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)
    sd = hig_amd.SpacedDiffusion(hig_amd.space_timesteps(N, 5), betas=gdm.get_named_beta_schedule("linear", N),
                                 model_mean_type=gdm.ModelMeanType.EPSILON, model_var_type=gdm.ModelVarType.FIXED_SMALL,
                                 loss_type=gdm.LossType.MSE)
    shape = tuple(x.shape)
    outs = (gd.p_sample_loop(g, shape, noise=x.clone(), clip_denoised=False, model_kwargs=kw, device="cpu"),
            sd.p_sample_loop(g, shape, noise=x.clone(), clip_denoised=False, model_kwargs=kw, device="cpu"),
            sd.ddim_sample_loop(g, shape, noise=x.clone(), clip_denoised=False, model_kwargs=kw, device="cpu", eta=0.0),
            sd.ddim_sample(g, x.clone(), torch.full((B,), 3), model_kwargs=kw)["sample"],
            gd.p_sample(g, x.clone(), torch.full((B,), 3), model_kwargs=kw)["sample"])
    assert all(o.shape == shape and torch.isfinite(o).all() for o in outs)
    assert m.calls == [2 * B] * (50 + 5 + 5 + 1 + 1)
    with pytest.raises(NotImplementedError):                          # classifier guidance stays out of scope
        sd.ddim_sample(g, x.clone(), torch.full((B,), 3), model_kwargs=kw, cond_fn=lambda *a, **k: 0)


# ---- 3. caption dropout ------------------------------------------------------------------------------------------------------
CAPS = ["a person waves", "two people hug", "a person jumps", "a person sits down", "a person runs"]


class Core:
    def to(self, _):
        return self

    def generate_src_mask(self, T, length):
        return torch.ones(len(length), T)


def single_trainer(prob, **extra):
    tr = hig_amd.DDPMTrainer.__new__(hig_amd.DDPMTrainer)
    tr.opt = types.SimpleNamespace(**extra) if prob is None else types.SimpleNamespace(cond_drop_prob=prob, **extra)
    tr.device, tr.encoder = torch.device("cpu"), Core()
    tr.sampler = types.SimpleNamespace(sample=lambda n, dev: (torch.zeros(n, dtype=torch.int64), None))
    seen = []
    tr.diffusion = types.SimpleNamespace(training_losses=lambda model, x_start, t, model_kwargs, **k: (
        seen.append(list(model_kwargs["text"])), dict(target=x_start, pred=x_start))[1])
    tr.clip_inputs = lambda caption: (seen.append(list(caption)), (None, None))[1]
    tr.train_step_fused = lambda *a, **k: None
    return tr, seen


def single_batch(n=len(CAPS)):
    return CAPS[:n], torch.zeros(n, 4, 3), torch.full((n,), 4)


def pair_trainer(prob, with_label):
    tr = hig_amd.DDPMMulTrainer.__new__(hig_amd.DDPMMulTrainer)
    tr.opt = types.SimpleNamespace(cond_drop_prob=prob, cap_id=False)
    tr.device, tr.encoder = torch.device("cpu"), Core()
    tr.multi, tr.with_label, tr.cap_id = True, with_label, False
    tr.sampler = types.SimpleNamespace(sample=lambda n, dev: (torch.zeros(n, dtype=torch.int64), None))
    seen = []
    tr.diffusion = types.SimpleNamespace(training_losses=lambda model, x_start, t, model_kwargs, **k: (
        seen.append(list(model_kwargs["text"])), dict(target=x_start, pred=x_start))[1])
    tr.clip_inputs = lambda caption: (seen.append(list(caption)), (None, None))[1]
    tr.train_step_fused = lambda *a, **k: None
    return tr, seen


C1 = ["one waves", "one bows", "one pushes", "one kicks"]
C2 = ["two waves back", "two bows back", "two falls", "two dodges"]


def pair_batch():
    n = len(C1)
    return C1, C2, torch.zeros(n, 4, 3), torch.zeros(n, 4, 3), torch.full((n,), 4)


@pytest.mark.parametrize("entry", ("forward", "train_fused_batch"))
def test_cond_drop_prob_single_person(entry):
    for prob in (None, 0.0):                       # absent or 0: the captions and the generator are left alone
        tr, seen = single_trainer(prob)
        torch.manual_seed(11)
        before = torch.get_rng_state()
        getattr(tr, entry)(single_batch())
        assert seen == [CAPS] and torch.equal(torch.get_rng_state(), before)
    tr, seen = single_trainer(1.0)
    getattr(tr, entry)(single_batch())
    assert seen == [[""] * len(CAPS)]
    tr, seen = single_trainer(0.5)
    torch.manual_seed(12)
    keep = (torch.rand(len(CAPS)) >= 0.5).tolist()                  # the ONE draw the step makes, on the CPU generator
    after = torch.get_rng_state()
    assert 0 < sum(keep) < len(CAPS)                                # (this seed drops some and keeps some)
    torch.manual_seed(12)
    getattr(tr, entry)(single_batch())
    assert seen == [[c if k else "" for c, k in zip(CAPS, keep)]]
    assert torch.equal(torch.get_rng_state(), after)                # exactly one torch.rand(n)
    for bad in (-0.1, 1.5, float("nan")):
        tr, _ = single_trainer(bad)
        with pytest.raises(ValueError):
            getattr(tr, entry)(single_batch())
    tr, _ = single_trainer(0.5, cap_id=True)
    with pytest.raises(NotImplementedError):
        getattr(tr, entry)(single_batch())


@pytest.mark.parametrize("with_label", (True, False))
@pytest.mark.parametrize("entry", ("forward", "train_fused_batch"))
def test_cond_drop_prob_two_person_is_per_pair(entry, with_label):
    n = len(C1)
    order = (lambda a, b: a + b) if with_label else (lambda a, b: a + b + b + a)     # PIT: (c1, c2, c2, c1)
    tr, seen = pair_trainer(0.0, with_label)
    torch.manual_seed(21)
    before = torch.get_rng_state()
    getattr(tr, entry)(pair_batch())
    assert seen == [order(C1, C2)] and torch.equal(torch.get_rng_state(), before)
    tr, seen = pair_trainer(1.0, with_label)
    getattr(tr, entry)(pair_batch())
    assert seen == [[""] * len(order(C1, C2))]
    tr, seen = pair_trainer(0.5, with_label)
    torch.manual_seed(20)
    keep = (torch.rand(n) >= 0.5).tolist()                          # one draw per PAIR
    after = torch.get_rng_state()
    assert 0 < sum(keep) < n
    torch.manual_seed(20)
    getattr(tr, entry)(pair_batch())
    d1, d2 = [c if k else "" for c, k in zip(C1, keep)], [c if k else "" for c, k in zip(C2, keep)]
    assert seen == [order(d1, d2)] and torch.equal(torch.get_rng_state(), after)
    tr, _ = pair_trainer(0.5, with_label)
    tr.opt.cap_id = tr.cap_id = True
    with pytest.raises(NotImplementedError):
        getattr(tr, entry)(pair_batch())


# ---- 4. set_sampler ----------------------------------------------------------------------------------------------------------
def sampler_trainer(cls=None):
    cls = cls or hig_amd.DDPMTrainer
    tr = cls.__new__(cls)
    tr.diffusion_steps = N
    tr.diffusion = hig_amd.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", N),
                                             model_mean_type=gdm.ModelMeanType.EPSILON,
                                             model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)
    tr._few_step, tr._guidance_scale = None, None
    tr.device = torch.device("cpu")
    return tr


def test_set_sampler_guidance_scale_validation():
    tr = sampler_trainer()
    for bad in (float("nan"), float("inf"), -float("inf"), "much"):
        with pytest.raises(ValueError):
            tr.set_sampler(steps=10, method="ddim", guidance_scale=bad)
    assert tr._guidance_scale is None and tr._few_step is None
    tr.set_sampler(guidance_scale=2.5)                              # kept independently of steps: the full chain, guided
    assert tr._few_step is None and tr._guidance_scale == 2.5
    tr.set_sampler(steps=10, method="ddim", guidance_scale=7)
    assert tr._few_step[0].num_timesteps == 10 and tr._guidance_scale == 7.0
    tr.set_sampler(steps=10, method="ddim")
    assert tr._guidance_scale is None                               # the default resets it
    tr.set_sampler(guidance_scale=0.0)
    assert tr._guidance_scale == 0.0                                # 0 is a scale (the unconditional sample), not "off"
    mt = sampler_trainer(hig_amd.DDPMMulTrainer)
    mt.cap_id = True
    with pytest.raises(NotImplementedError):
        mt.set_sampler(steps=10, method="ddim", guidance_scale=2.5)
    mt.set_sampler(steps=10, method="ddim", guidance_scale=1.0)     # unguided: nothing to refuse


@pytest.mark.parametrize("scale", (None, 1.0, 2.5))
@pytest.mark.parametrize("sampler", (None, "ddim", "ddpm"))
def test_sample_loop_wraps_the_encoder_only_with_a_scale(scale, sampler):
    tr = sampler_trainer()
    encoded = []

    class Enc:
        def encode_text(self, text, device):
            encoded.append(list(text))
            return torch.ones(len(text), 8), torch.ones(len(text), 3, 8)

    tr.encoder = Enc()
    tr.set_sampler(steps=None if sampler is None else 10, method=sampler or "ddpm", guidance_scale=scale)
    seen = []
    spy = lambda model, shape, **kw: (seen.append((model, kw)), torch.zeros(shape))[1]  # noqa: E731
    tr.diffusion.p_sample_loop = spy
    if tr._few_step is not None:
        tr._few_step[0].p_sample_loop = tr._few_step[0].ddim_sample_loop = spy
    known, mask = torch.zeros(6, 4, 5), torch.ones(6, 4, 5, dtype=torch.bool)
    tr._sample_loop((6, 4, 5), dict(xf_proj=None, xf_out=None, length=None), known, mask)
    (model, kw), = seen
    assert kw["known"] is known and kw["known_mask"] is mask and kw["clip_denoised"] is False      # passed through unchanged
    if scale in (None, 1.0):
        assert model is tr.encoder and encoded == []                # the encoder itself: launch for launch the unguided loop
    else:
        assert isinstance(model, hig_amd.ClassifierFreeGuidedModel) and model.model is tr.encoder and model.scale == scale
        assert encoded == [[""]]                                    # the empty caption, encoded once ...
        assert model.uncond_kwargs["xf_proj"].shape == (6, 8) and model.uncond_kwargs["xf_out"].shape == (6, 3, 8)   # ... expanded
        assert model.group == 6


def test_two_person_trainer_groups_by_pairs():
    mt = sampler_trainer(hig_amd.DDPMMulTrainer)
    mt.multi, mt.cap_id = True, False
    mt.encoder = types.SimpleNamespace(encode_text=lambda text, device: (torch.ones(1, 8), torch.ones(1, 3, 8)))
    mt.set_sampler(steps=10, method="ddim", guidance_scale=2.5)
    assert mt._guided_encoder(6).group == 3
