"""Drop-in mirror of the reference's frequency-separation trainer (reference DoWnGAN/GAN/wasserstein_fs.py:15-198).

``WassersteinGANFS(G, C, G_optimizer, C_optimizer)``: same interface as ``WassersteinGAN``; the critic is trained on the
high-pass parts ``x - low(x)`` of the real and generated fields and the content loss on the low-pass parts, with
``low = AvgPool2d(5, 1, 0) o ReplicationPad2d(2)`` (hyperparams.py:31-35).  The reference module itself is not importable
(broken imports, wasserstein_fs.py:2-10) and nothing reads ``hp.freq_sep``; this follows the text of its iteration methods.
"""
from __future__ import annotations

from ..engine import TrainEngineFS
from .wasserstein import WassersteinGAN


class WassersteinGANFS(WassersteinGAN):
    engine_class = TrainEngineFS
