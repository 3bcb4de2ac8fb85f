"""BaseGAN: device selection and checkpoint I/O (reference GAN_models/baseGAN.py:19-106).

Checkpoint layout is the reference's: ``G_{it}.pth`` / ``D_{it}.pth`` hold plain
``state_dict``s (same keys, logical (Cout, Cin, kx, ky, kz) fp32 filters) and
``state_{it}.pth`` = ``{"it", "epoch", "schedulers": [...], "optimizers": [...]}``.

With the moving average of the generator's weights on ([EMA], ``init_ema``) there is also ``G_ema_{it}.pth``: the
shadows as a plain state dict with the keys and shapes of ``G_{it}.pth``, so it loads wherever that file loads.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from ..tools import loggingclass as lc


def _given(path) -> bool:
    return path is not None and str(path).lower() not in ("null", "none")


def ema_path_of(generator_path: str) -> str:
    """``.../G_<n>.pth`` -> ``.../G_ema_<n>.pth`` (any other file name: ``ema_`` in front of it)"""
    folder, name = os.path.split(str(generator_path))
    return os.path.join(folder, "G_ema_" + name[2:] if name.startswith("G_") else "ema_" + name)


class BaseGAN(lc.GlobalLoggingClass):
    G: nn.Module = None
    D: nn.Module = None

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        # ONE source of truth for the device: ``cfg.device`` when a launcher set it (run.py / train.py put
        # every rank on cuda:LOCAL_RANK), else the reference's rule ``cuda:{gpu_id}`` (baseGAN.py:27-33).
        dev = getattr(cfg, "device", None)
        if dev is not None:
            self.device = torch.device(dev)
        else:
            use_gpu = torch.cuda.is_available() and cfg.gpu_id is not None
            self.device = torch.device(f"cuda:{cfg.gpu_id}") if use_gpu else torch.device("cpu")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.is_train = cfg.is_train
        self.schedulers = []
        self.optimizers = []
        self.ema_shadows: Optional[List[torch.Tensor]] = None  # None: no moving average of G's weights
        self._in_ema_scope = False

    # ------------------------------------------------------------------ moving average of the generator's weights
    def init_ema(self) -> List[torch.Tensor]:
        """one shadow per parameter of G (``G.parameters()`` order, the optimizer's), starting as copies"""
        self.ema_shadows = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.G.parameters()]
        return self.ema_shadows

    def reset_ema(self) -> None:
        """shadows = the generator's current weights (after the weights were replaced behind the average's back)"""
        with torch.no_grad():
            for e, p in zip(self.ema_shadows, self.G.parameters()):
                e.copy_(p)

    def G_ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """the shadows under the generator's ``state_dict`` keys (a buffer, which is not averaged, as it is)"""
        if self.ema_shadows is None:
            raise RuntimeError("the moving average of the generator's weights is off (no [EMA] section)")
        if self._in_ema_scope:
            raise RuntimeError("G_ema_state_dict inside ema_scope(): there G.state_dict() holds the averaged weights")
        by_name = {name: e for (name, _), e in zip(self.G.named_parameters(), self.ema_shadows)}
        return {k: by_name[k].detach() if k in by_name else v for k, v in self.G.state_dict().items()}

    def _swap_ema(self) -> None:
        for p, e in zip(self.G.parameters(), self.ema_shadows):  # storage pointers change hands: nothing is copied
            p.data, e.data = e.data, p.data
        program = getattr(self.G, "program", None)
        if callable(program):  # packed compute copies of the filters must not survive the swap
            program().filters.invalidate()

    @contextlib.contextmanager
    def ema_scope(self):
        """Inside, the generator runs with the averaged weights: parameters and shadows swap storage on entry and swap
        back on exit (also when the body raises).  No optimizer step belongs in here; nested entry is refused."""
        if self.ema_shadows is None:
            raise RuntimeError("the moving average of the generator's weights is off (no [EMA] section)")
        if self._in_ema_scope:
            raise RuntimeError("ema_scope() is already entered")
        self._swap_ema()
        self._in_ema_scope = True
        try:
            yield self
        finally:
            self._swap_ema()
            self._in_ema_scope = False

    def load_model(self, generator_load_path: str = None, discriminator_load_path: str = None,
                   state_load_path: str = None):
        """Returns ``(epoch, it)`` when a training state was loaded, else ``(None, None)``."""
        if _given(generator_load_path):
            self.G.load_state_dict(torch.load(generator_load_path, map_location="cpu"))
            self.G.eval()
            if self.ema_shadows is not None:
                ema_path = ema_path_of(generator_load_path)
                if os.path.isfile(ema_path):
                    sd = torch.load(ema_path, map_location="cpu")
                    with torch.no_grad():
                        for (name, _), e in zip(self.G.named_parameters(), self.ema_shadows):
                            e.copy_(sd[name])
                    self.status_logs.append(f"EMA: loaded the averaged generator weights from {ema_path}")
                else:
                    self.reset_ema()
                    self.status_logs.append(f"EMA: no {ema_path}; the average starts from the weights of "
                                            f"{generator_load_path}")
        if _given(discriminator_load_path):
            self.D.load_state_dict(torch.load(discriminator_load_path, map_location="cpu"))
            self.G.eval()
        if _given(state_load_path):
            state = torch.load(state_load_path)
            opts, scheds = state["optimizers"], state["schedulers"]
            assert len(opts) == len(self.optimizers), \
                f"Loaded {len(opts)} optimizers but expected {len(self.optimizers)}"
            assert len(scheds) == len(self.schedulers), \
                f"Loaded {len(scheds)} schedulers but expected {len(self.schedulers)}"
            for mine, theirs in zip(self.optimizers, opts):
                mine.load_state_dict(theirs)
            for mine, theirs in zip(self.schedulers, scheds):
                mine.load_state_dict(theirs)
            return state["epoch"], state["it"]
        return None, None

    def save_model(self, save_basepath: str, epoch: int, it: int, save_G: bool = True, save_D: bool = True,
                   save_state: bool = True):
        folder = self.cfg.env.this_runs_folder  # the argument is ignored, as in the reference (:91)
        if save_G:
            torch.save(self.G.state_dict(), os.path.join(folder, f"G_{it}.pth"))
            if self.ema_shadows is not None:
                torch.save(self.G_ema_state_dict(), os.path.join(folder, f"G_ema_{it}.pth"))
        if save_D:
            torch.save(self.D.state_dict(), os.path.join(folder, f"D_{it}.pth"))
        if save_state:
            state = {"it": it, "epoch": epoch,
                     "schedulers": [s.state_dict() for s in self.schedulers],
                     "optimizers": [o.state_dict() for o in self.optimizers]}
            torch.save(state, os.path.join(folder, f"state_{it}.pth"))
