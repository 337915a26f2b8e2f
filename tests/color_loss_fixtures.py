"""TEST INFRASTRUCTURE ONLY -- fixtures of the colour-loss tests: the protocol that drives a trainer with the three image-space terms on
(`drive_with_color_losses`: what tests/golden/trainer_C*.npz holds), the reference's flags for it and the loader of
tests/golden/color_loss_<tag>.npz.  The float64 contract itself is oracle/contracts.color_terms.
"""
import parity_utils as PU

COLOR_KEYS = ("background", "rgb", "lab")


class _ColorRecorder:
    """A trainer proxy that notes the three image-space losses after every generator step (oracle.trainer_parity.drive keeps
    its own fixed list of loss keys)."""

    def __init__(self, trainer):
        self.__dict__["_tr"], self.__dict__["seen"] = trainer, []

    def __getattr__(self, name):
        return getattr(self._tr, name)

    def run_generator_one_step(self, data):
        self._tr.run_generator_one_step(data)
        self.seen.append({k: float(self._tr.g_losses[k].detach().float().mean()) for k in COLOR_KEYS})


def drive_with_color_losses(trainer, cfg, device="cpu"):
    """oracle.trainer_parity.drive's record + it<i>.loss.{background,rgb,lab}: what tests/golden/trainer_C.npz holds."""
    import numpy as np
    from oracle import trainer_parity as TP
    rec_tr = _ColorRecorder(trainer)
    rec = TP.drive(rec_tr, cfg, device=device)
    for it, vals in enumerate(rec_tr.seen):
        for k, v in vals.items():
            rec["it%d.loss.%s" % (it, k)] = np.array(v)
    return rec


def color_argv(cfg, checkpoints_dir):
    """The README training flags AS PUBLISHED (Lab on) plus background and rgb on: oracle.trainer_parity.reference_argv
    without the three switches that turn the terms off."""
    from oracle import trainer_parity as TP
    return [a for a in TP.reference_argv(cfg, checkpoints_dir) if a not in ("--no_lab_loss", "--no_background_loss", "--no_rgb_loss")]


def load_pair(tag):
    """tests/golden/color_loss_<tag>.npz as tensors (scalars as Python numbers)."""
    return PU.load_tensors("color_loss_%s.npz" % tag)
