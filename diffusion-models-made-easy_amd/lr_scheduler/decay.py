"""Linear learning-rate decay to zero over one stage of progressive distillation (Salimans & Ho 2022: the rate is annealed linearly
to zero within every halving stage); stepped once per training step like `WarmupLR`."""

from torch.optim.lr_scheduler import LRScheduler


class LinearDecayLR(LRScheduler):
    def __init__(self, optimizer, total_steps, last_epoch=-1):
        if int(total_steps) < 1:
            raise ValueError(f"total_steps = {total_steps!r}; a stage has at least one step")
        self.total_steps = int(total_steps)
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        # steps already taken, counted like WarmupLR counts them: step k + 1 of a stage runs at (1 - k / total_steps) of the initial rate
        done = getattr(self.optimizer, "_step_count", self._step_count - 1)
        scale = max(0.0, 1.0 - done / self.total_steps)
        return [g["initial_lr"] * scale for g in self.optimizer.param_groups]
