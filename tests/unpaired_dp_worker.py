"""One rank of the data-parallel unpaired-stage check of tests/test_unpaired.py (spawned by it; not a test module itself):
gloo on the CPU, the C-ABI contract emulator as backend.  One generator + discriminator step at curr_step = 2 with unpairTrain; rank r
feeds sample r of the seeded unpaired loader batch.  Afterwards netG and netD2 must be bit-identical on the two ranks (the broadcast
aligned them, the gradient all-reduce kept them aligned) and netD must be exactly what the broadcast left."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(2)
    from michigan_amd import _cabi, parallel
    from michigan_amd.model import Pix2PixTrainer
    from michigan_amd.synth import synth_loader_batch
    from oracle import trainer_parity as TP
    from oracle.cabi_emulator import EmulatorBackend
    be = EmulatorBackend()
    _cabi.set_backend(be)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64)
    torch.manual_seed(rank)                                    # different initial weights per rank: the broadcast has to align them
    trainer = Pix2PixTrainer(TP.repo_options(cfg, unpairTrain=True, curr_step=2))
    assert trainer.optimizer_D2 is not None and trainer.optimizer_D2.dp and parallel.world_size() == world
    m = trainer.pix2pix_model_on_one_gpu
    state = lambda net: {k: v.detach().clone() for k, v in net.state_dict().items()}
    d_before, d2_before, g_before = state(m.netD), state(m.netD2), state(m.netG)
    data = synth_loader_batch(cfg["n"], cfg["crop"], seed=cfg["seed_x"], unpaired=True)
    per = cfg["n"] // world
    cut = lambda v: v[rank * per:(rank + 1) * per]
    mine = lambda: {k: (cut(v).clone() if torch.is_tensor(v) else cut(v)) for k, v in data.items()}
    parallel.seed_shared_rng(cfg["seed_py"])
    trainer.run_generator_one_step(mine())
    parallel.seed_shared_rng(cfg["seed_py"] + 1)
    trainer.run_discriminator_one_step(mine())
    ok = {"keys": sorted(trainer.get_latest_losses()), "hair_fwd": list(be.flags("mg_hair_lab_fwd")), "hair_bwd": list(be.flags("mg_hair_lab_bwd"))}
    ok["netD_untouched"] = all(torch.equal(v, d_before[k]) for k, v in m.netD.state_dict().items())
    ok["netD2_moved"] = any(not torch.equal(v, d2_before[k]) for k, v in m.netD2.named_parameters())
    ok["netG_moved"] = any(not torch.equal(v, g_before[k]) for k, v in m.netG.named_parameters())
    same = True
    for net in (m.netG, m.netD2, m.netD):
        for _, t in list(net.named_parameters()) + list(net.named_buffers()):
            ref = t.detach().clone()
            dist.broadcast(ref, src=0)
            same = same and torch.equal(ref, t.detach())
    ok["replicas_identical"] = same
    q.put((rank, ok))
    dist.barrier()
    parallel.shutdown()
    dist.destroy_process_group()
