"""ONE rank on the real RCCL backend for tests/test_gpu_class_head.py, as tests/rccl_worker.py is for tests/test_gpu_rccl.py:
`init_process_group("nccl", world_size=1)` with HIG_FORCE_EXCHANGE=1, so that the fused and the captured step of a cap_id model
with the HIP class head really issue their gradient all-reduces -- the per-layer ones, and the tail range (core_numel, n) that
now holds the class head's gradients.  An all-reduce over one rank is the identity: every number must equal the same steps
without a process group, bit for bit.
usage: class_head_worker.py <port> <outdir>"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

CASE = dict(B=2, T=33, F=20, d=256, H=4, L=2, ff=256, N=77, Lt=64, num_frames=40, lengths=(33, 12), t=(4, 700))
PIT_IDS = ([3, 41, 4, 3, 4, 3, 3, 41], [7, 7, 0, 42, 0, 42, 7, 7])       # rows c1, c2, c2, c1 of two different steps


def pit_trainer(c, storage="f32", label_path=None, **opt):
    import hig_amd
    from oracle import fill
    m = hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                             num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], storage=storage,
                                             cap_id=True, class_head=opt.pop("class_head", "hip"))
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    m = m.to("cuda").train()
    args = types.SimpleNamespace(device=torch.device("cuda"), diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=c["B"],
                                 num_epochs=1, log_every=50, save_latest=500, save_every_e=5, is_continue=False, model_dir="/tmp",
                                 multi=True, label_path=label_path, cap_id=True, **opt)
    return hig_amd.DDPMMulTrainer(args, m), m


def exchange_steps():
    """Two eager fused steps and two captured ones (the second replay with other ids), PIT mode; what the test compares."""
    from oracle import fill
    c = CASE
    tr, m = pit_trainer(c)
    B = c["B"]
    x0 = (fill.tensor_for("cls.rccl.x0", (2 * B, c["T"], c["F"])) * 10).to("cuda")
    noise = [(fill.tensor_for("cls.rccl.nz.%d" % k, x0.shape) * 10).to("cuda") for k in range(2)]
    tt, length = torch.tensor(c["t"], device="cuda"), torch.tensor(c["lengths"], device="cuda")
    ids = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in PIT_IDS]
    losses = [step(x0, tt, length, noise=noise[k], class_ids=ids[k]).item()
              for step in (tr.train_step_fused, tr.train_step_captured) for k in range(2)]
    torch.cuda.synchronize()
    st, fp = tr.fused_state(), m.flat_params()
    return {"flat": fp.flat.cpu(), "m": st["m"].cpu(), "v": st["v"].cpu(), "losses": losses, "gnorm": st["gnorm"].item(),
            "step": st["step"].item(), "captured_form": st.get("captured_form"), "numel": fp.numel, "core_numel": fp.core_numel,
            "L": c["L"]}


def main():
    port, outdir = sys.argv[1], sys.argv[2]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK="0", WORLD_SIZE="1", HIG_FORCE_EXCHANGE="1")
    import torch.distributed as dist
    from hig_amd import parallel

    def body(rank, world):
        assert dist.get_backend() == "nccl" and world == 1 and parallel.exchange_active()
        body.count = 0
        out = exchange_steps()
        out["n_allreduce"] = body.count
        torch.save(out, os.path.join(outdir, "class_head.pt"))

    body.count = 0
    real = dist.all_reduce

    def counting(*a, **k):
        body.count += 1
        return real(*a, **k)
    dist.all_reduce = counting
    parallel.run_distributed(body, 0, 1, "nccl")


if __name__ == "__main__":
    main()
