"""What the fp8 convolutions (ops/conv.py) and the fp8 Linear layers (ops/linear.py) share: the launch
counters and the MX weight operand lookup."""
from __future__ import annotations

import torch

# fp8 kernel launches by role (tests / logs): "fwd" / "dgrad" the convolutions, "lin_fwd" / "lin_dgrad" the
# Linear layers ("lin_wgrad" their fp8 weight gradients, feature ``fp8_wgrad``), "ps_weights" forwards (of
# either) that read the MX weight copy the PS data plane published
FP8_CALLS = {"fwd": 0, "dgrad": 0, "ps_weights": 0, "lin_fwd": 0, "lin_dgrad": 0, "lin_wgrad": 0}


def mx_weight(mod, w2: torch.Tensor):
    """MX e4m3 forward weight operand ``(q [out, K], E8M0 scales)`` of ``w2``: the copy the PS data plane
    published with the weights this step's forward uses (``_psd_w8``, parallel/flat.py
    install_fp8_weights: no per-step weight quantisation), else quantised here."""
    pub = getattr(mod, "_psd_w8", None) if mod is not None else None
    got = pub(w2) if pub is not None else None
    if got is not None:
        FP8_CALLS["ps_weights"] += 1
        return got
    from . import quantize_mx

    return quantize_mx(w2)
