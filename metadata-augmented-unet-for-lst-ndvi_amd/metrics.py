"""Running train-loss trackers of the step log (the reference's ``RunningLoss``, src/utils/metrics.py): host arithmetic only."""
from collections import deque


class RunningLoss:
    """``mode='cumulative'``: sample-weighted mean of everything seen; ``'ema'``: ``alpha * old + (1 - alpha) * new``, seeded with
    the first value; ``'sma'``: mean of the last ``window_size`` values (a value counts ``n`` times).  ``update`` returns the new
    value, ``get`` the current one (``None`` for an ema that has seen nothing)."""

    def __init__(self, mode: str = "cumulative", window_size: int = 100, ema_alpha: float = 0.98):
        if mode not in ("cumulative", "ema", "sma"):
            raise ValueError(f"Unknown mode {mode}")
        self.mode, self.window_size, self.ema_alpha = mode, window_size, ema_alpha
        self.reset()

    def reset(self):
        self.total, self.count, self.value = 0.0, 0, None if self.mode == "ema" else 0.0
        self.window = deque(maxlen=self.window_size)

    def update(self, val: float, n: int = 1) -> float:
        if self.mode == "cumulative":
            self.total, self.count = self.total + val * n, self.count + n
            self.value = self.total / (self.count + 1e-12)
        elif self.mode == "ema":
            self.value = val if self.value is None else self.ema_alpha * self.value + (1 - self.ema_alpha) * val
        else:
            self.window.extend([val] * n)
            self.value = sum(self.window) / (len(self.window) + 1e-12)
        return self.value

    def get(self):
        return self.value
