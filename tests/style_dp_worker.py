"""One rank of the data-parallel check of tests/test_style_loss.py (spawned by it; not a test module itself): gloo on the CPU, the
C-ABI contract emulator as backend.  Rank r computes the style / content terms of sample r of feature set i; the mean over the ranks
(what the gradient all-reduce of a one-process-per-GPU job forms) must be the one-rank value on the concatenated batch for the unmasked
terms, loss and gradient.  The masked content term divides by its OWN replica's mask sum, as each replica of the reference's
DataParallel does: there the mean over the ranks is not the concatenated batch's value."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(2)
    import style_loss_fixtures as SE
    from michigan_amd import _cabi, ops
    from oracle import contracts as K
    from oracle.cabi_emulator import EmulatorBackend
    _cabi.set_backend(EmulatorBackend())
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    p = SE.make_sets()["i"]
    assert p["x"].shape[0] == world
    mine = {k: v[rank:rank + 1] for k, v in p.items()}
    view = lambda f: f.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)

    def terms(d, masked):
        x = view(d["x"]).requires_grad_(True)
        masks = [d[k] for k in ("mask_x", "mask_s", "mask_t")] if masked else [None] * 3
        style, content = ops.feat_moment_loss(x, view(d["s"]), view(d["t"]), *masks, flags=3)
        (SE.WEIGHTS[0] * style + SE.WEIGHTS[1] * content).backward()
        return torch.stack([style.detach(), content.detach()]).double(), x.grad.double()

    ok = {}
    losses, grad = terms(mine, False)
    mean = losses.clone()
    dist.all_reduce(mean)
    mean /= world
    whole_l, whole_g = K.style_terms(p["x"], p["s"], p["t"], flags=3, weights=SE.WEIGHTS)
    ok["plain_matches"] = bool(((mean - whole_l).abs() <= 1e-6 * whole_l.abs()).all())
    ok["grad_matches"] = float((grad / world - whole_g[rank:rank + 1]).norm() / whole_g[rank:rank + 1].norm()) <= 1e-6
    losses, _ = terms(mine, True)
    own = K.style_terms(mine["x"], mine["s"], mine["t"], mine["mask_x"], mine["mask_s"], mine["mask_t"], flags=3)[0]
    mean = losses.clone()
    dist.all_reduce(mean)
    mean /= world
    whole = K.style_terms(p["x"], p["s"], p["t"], p["mask_x"], p["mask_s"], p["mask_t"], flags=3)[0]
    ok["masked_content_is_per_replica"] = bool(abs(float(losses[1] - own[1])) <= 1e-6 * float(own[1])) and \
        abs(float(mean[1] - whole[1])) > 1e-4 * float(whole[1]) and float(p["mask_t"][0].sum()) != float(p["mask_t"][1].sum())
    q.put((rank, ok))
    dist.barrier()
    dist.destroy_process_group()
