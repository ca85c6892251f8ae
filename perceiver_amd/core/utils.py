"""Small building blocks shared by all Perceiver models.

Functional parity with /root/reference/perceiver/model/core/utils.py (ModuleOutput,
Residual, init_parameters, freeze) — reimplemented for the MI355X-native stack.
State-dict key layout (``module.*`` inside Residual) is kept compatible with the
reference checkpoint format.
"""
from __future__ import annotations

import os
from collections import OrderedDict

import torch
import torch.nn as nn


class ModuleOutput(OrderedDict):
    """Ordered dict with attribute access; the uniform return type of all core modules."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(f"No such attribute: {name}") from None

    def __setattr__(self, name, value):
        self[name] = value

    def __delattr__(self, name):
        try:
            del self[name]
        except KeyError:
            raise AttributeError(f"No such attribute: {name}") from None


# Register with torch's pytree so containers of tensors returned by module
# forwards are traversed (FSDP2 attaches its pre-backward re-gather hooks to the
# tensors it finds in the output tree; an unregistered OrderedDict SUBCLASS is a
# leaf and the hooks would silently not attach).
torch.utils._pytree.register_pytree_node(
    ModuleOutput,
    lambda mo: (list(mo.values()), list(mo.keys())),
    lambda values, keys: ModuleOutput(zip(keys, values)),
)


class PendingResidual:
    """The two halves of a residual block whose sum has not been formed: the branch
    output ``hidden`` and the ``shortcut``. A residual block hands this pair to its
    successor, whose first LayerNorm forms the sum and normalises it in one pass
    (:func:`perceiver_amd.ops.norm.add_layer_norm`); wherever a chain of blocks ends
    the pair is materialised with a plain add."""

    __slots__ = ("hidden", "shortcut")

    def __init__(self, hidden: torch.Tensor, shortcut: torch.Tensor):
        self.hidden = hidden
        self.shortcut = shortcut

    def materialize(self) -> torch.Tensor:
        return self.hidden + self.shortcut


# A layer may return the pair: FSDP2 must find its two tensors like any others.
torch.utils._pytree.register_pytree_node(
    PendingResidual,
    lambda p: ([p.hidden, p.shortcut], None),
    lambda values, _: PendingResidual(*values),
)


def materialize(x):
    """The tensor behind ``x``: the sum of a pending residual pair, or ``x`` itself."""
    return x.materialize() if isinstance(x, PendingResidual) else x


def fused_residual_enabled() -> bool:
    """PERCEIVER_FUSED_RESIDUAL=0 restores the add-then-LayerNorm path everywhere."""
    return os.environ.get("PERCEIVER_FUSED_RESIDUAL", "1") != "0"


class Residual(nn.Module):
    """Residual connection around ``module`` with dropout on the module output.

    ``module`` must return a :class:`ModuleOutput`; the residual is added to its
    ``last_hidden_state`` and the (possibly present) ``kv_cache`` is passed through.

    Residual-stream hand-over: a ``module`` that names its leading LayerNorm
    (``residual_norm``) and can run on an already normalised input
    (``forward_prenormed``) lets this block take a :class:`PendingResidual` as its
    first argument, form the pending sum inside that LayerNorm, and keep the sum as
    its own shortcut. With ``defer=True`` the block returns its own (hidden,
    shortcut) pair instead of their sum, for a successor that does the same. Only
    without residual dropout and without a kv cache; a ``defer`` that cannot be
    honoured returns the sum as always.
    """

    def __init__(self, module: nn.Module, dropout: float = 0.0):
        super().__init__()
        self.module = module
        self.dropout = nn.Dropout(dropout)
        # cleared by activation_checkpoint_wrapper: a checkpointed layer keeps the
        # plain add-then-LayerNorm path
        self.handover = True

    def _hands_over(self, kwargs) -> bool:
        return (
            self.handover
            and fused_residual_enabled()
            and not (self.training and self.dropout.p > 0.0)
            and kwargs.get("kv_cache") is None
            and hasattr(self.module, "forward_prenormed")
        )

    def forward(self, *args, defer: bool = False, **kwargs):
        if self._hands_over(kwargs):
            from perceiver_amd.ops.norm import add_layer_norm

            x = args[0]
            pending = isinstance(x, PendingResidual)
            shortcut, normed = add_layer_norm(
                self.module.residual_norm,
                x.hidden if pending else None,
                x.shortcut if pending else x,
            )
            output = self.module.forward_prenormed(normed, *args[1:], **kwargs)
            hidden = output.last_hidden_state
            output.last_hidden_state = (
                PendingResidual(hidden, shortcut) if defer else hidden + shortcut
            )
            return output

        args = (materialize(args[0]),) + args[1:]
        output = self.module(*args, **kwargs)
        hidden = output.last_hidden_state
        shortcut = args[0]
        p = self.dropout.p
        if _fused_dropout_add_ok(hidden, shortcut, p, self.training):
            from perceiver_amd.ops.dropadd import dropout_add

            output.last_hidden_state = dropout_add(hidden, shortcut, p)
        else:
            output.last_hidden_state = self.dropout(hidden) + shortcut
        return output


def _fused_dropout_add_ok(hidden, shortcut, p, training) -> bool:
    if not (training and p > 0.0 and hidden.is_cuda):
        return False
    from perceiver_amd.ops.dropadd import can_use_dropout_add

    return can_use_dropout_add(hidden, shortcut, p, training)


def init_parameters(module: nn.Module, init_scale: float) -> None:
    """Normal(0, init_scale) init of every Linear/Embedding weight; zero biases."""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            m.weight.data.normal_(mean=0.0, std=init_scale)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.Embedding):
            m.weight.data.normal_(mean=0.0, std=init_scale)


def freeze(module: nn.Module) -> None:
    for p in module.parameters():
        p.requires_grad = False
