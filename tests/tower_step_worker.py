"""The model, trainer and inputs of tests/test_gpu_tower_step.py's step tests, and -- run as a program -- ONE rank on the real RCCL
backend, as tests/class_head_worker.py is for tests/test_gpu_class_head.py: `init_process_group("nccl", world_size=1)` with
HIG_FORCE_EXCHANGE=1, so that a fused step that trains the CLIP text tower really issues its gradient all-reduces -- the
per-layer ones and the tail range (core_numel, n), which now runs over the text head AND the tower.  An all-reduce over one rank
is the identity: every number must equal the same step without a process group, bit for bit.
usage: tower_step_worker.py <port> <outdir>"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

DEV = "cuda"
N = 77
TOWER = dict(W=512, H=8, L=2)          # the tower of tests/test_gpu_clip_train.py's build()
STEPS = 3
# three pairs in PIT mode: 12 text rows c1 + c2 + c2 + c1 per step, 4 .. 5 distinct captions (U_pad = 8), other captions every step
CAP1 = (["a person shakes hands with another person", "one pushes the other", "a person shakes hands with another person"],
        ["two people hug", "one pushes the other", "they bow to each other and then one of them walks slowly away to the left"],
        ["jump", "a person waves the right hand", "jump"])
CAP2 = (["a person receives a handshake", "one pushes the other", "one is pushed by the other"],
        ["two people hug", "one is pushed by the other", "a person receives a bow"],
        ["a person watches", "jump", "a person waves back with the left hand"])


def case():
    from oracle import fill
    return dict(fill.ICASES["config1x2"], L=fill.CASES["config1"]["L"], B=3, lengths=(61, 41, 33), t=(0, 500, 999))


def build(heads=None, **kw):
    """The `config1` two-person model with a trainable W 512, H 8, L 2 tower behind the stub tokenizer.  heads: the denoiser's
    head count where `config1`'s 8 (head dim 16) will not do -- bf16 storage takes head dim 64 or 128."""
    import clip_bounds as CB
    import hig_amd
    from hig_amd.models import clip_text as CT
    from hig_amd.models import stub_clip
    from oracle import fill
    c = case()
    weights = CB.tower_weights(TOWER["W"], TOWER["H"], TOWER["L"], N, stub_clip.VOCAB, seed=11)
    m = hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                             num_layers=c["L"], num_heads=heads or c["H"], text_latent_dim=c["Lt"], no_clip=True,
                                             clip_model=CT.load_text_tower(weights), clip_tokenize=stub_clip.tokenize, **kw)
    sd = fill.fill_state_dict(m.state_dict())
    sd.update({"clip." + k: v for k, v in weights.items()})      # (no_clip re-initialises the tower)
    m.load_state_dict(sd, strict=True)
    return m


def pit_trainer(m, **opt):
    import hig_amd
    c = case()
    args = types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=c["B"], num_epochs=1,
                                 log_every=50, save_latest=500, save_every_e=5, is_continue=False, model_dir="/tmp", multi=True,
                                 label_path=None, cap_id=False, **opt)
    return hig_amd.DDPMMulTrainer(args, m)


def motions(k):
    """(motion1, motion2) (B, T, F) and the noise (2 B, T, F) of step k, on the host."""
    from oracle import fill
    c = case()
    shape = (c["B"], c["T"], c["F"])
    return (fill.tensor_for("tower_step.m1.%d" % k, shape) * 10, fill.tensor_for("tower_step.m2.%d" % k, shape) * 10,
            fill.tensor_for("tower_step.noise.%d" % k, (2 * c["B"],) + shape[1:]) * 10.0)


def rows_of(k):
    """The 4 B captions of step k in the model batch's row order."""
    return list(CAP1[k]) + list(CAP2[k]) + list(CAP2[k]) + list(CAP1[k])


def fused_step(tr, m, k, dedup=True, captured=False, t=None):
    """Step k through train_step_fused / train_step_captured with the step's TokenBatch; returns the device loss."""
    from hig_amd.models import clip_text as CT
    c = case()
    m1, m2, noise = motions(k)
    tb = CT.TokenBatch(rows_of(k), m._tokenize, dedup=dedup).to(DEV)
    step = tr.train_step_captured if captured else tr.train_step_fused
    t = torch.tensor(c["t"], device=DEV) if t is None else t
    return step(torch.cat([m1, m2]).to(DEV), t, torch.tensor(c["lengths"], device=DEV), noise=noise.to(DEV), token_batch=tb)


def exchange_step():
    """One eager fused step that trains the tower; what the test compares."""
    m = build(clip_tower_train="flat").to(DEV).train()
    tr = pit_trainer(m)
    loss = fused_step(tr, m, 0).item()
    torch.cuda.synchronize()
    st, fp = tr.fused_state(), m.flat_params()
    return {"flat": fp.flat.cpu(), "m": st["m"].cpu(), "v": st["v"].cpu(), "loss": loss, "gnorm": st["gnorm"].item(),
            "step": st["step"].item(), "numel": fp.numel, "core_numel": fp.core_numel, "tower0": fp.tower_offsets[0], "L": case()["L"]}


def main():
    port, outdir = sys.argv[1], sys.argv[2]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK="0", WORLD_SIZE="1", HIG_FORCE_EXCHANGE="1")
    import torch.distributed as dist
    from hig_amd import parallel

    def body(rank, world):
        assert dist.get_backend() == "nccl" and world == 1 and parallel.exchange_active()
        body.count = 0
        out = exchange_step()
        out["n_allreduce"] = body.count
        torch.save(out, os.path.join(outdir, "tower_step.pt"))

    body.count = 0
    real = dist.all_reduce

    def counting(*a, **k):
        body.count += 1
        return real(*a, **k)
    dist.all_reduce = counting
    parallel.run_distributed(body, 0, 1, "nccl")


if __name__ == "__main__":
    main()
