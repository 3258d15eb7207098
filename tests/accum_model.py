"""numpy restatement of a sequence of dg_grad_accumulate calls (include/drakegpt_hip.h): the accumulator, the control words
{j, k, arrival, 0}, the running / mean loss and the micro-step word after every call.  Every operation is one fp32 operation, as
in the kernel (no scale, no FMA), so the comparison with the device is bitwise."""
import numpy as np


class AccumModel:
    def __init__(self, n: int, k: int, step: int = 0, scratch: int = 0):
        if k < 1:
            raise ValueError("k >= 1")
        self.n, self.k = n, k
        self.acc = np.zeros(n, dtype=np.float32)
        self.ctl = np.array([0, k, 0, 0], dtype=np.uint32)
        self.loss_out = np.zeros(2, dtype=np.float32)
        self.rng_state = np.array([0, 0, step, scratch], dtype=np.uint32)      # words 0, 1 (seed) and 3 are never touched

    def call(self, g: np.ndarray, loss=None) -> None:
        g = np.asarray(g, dtype=np.float32)
        assert g.shape == (self.n,)
        j, k = int(self.ctl[0]), self.k
        self.acc = g.copy() if j == 0 else (self.acc + g).astype(np.float32)          # j == 0: acc is not read
        if loss is not None:
            l = np.float32(loss)
            self.loss_out[0] = l if j == 0 else np.float32(self.loss_out[0] + l)
            if j == k - 1:
                self.loss_out[1] = np.float32(self.loss_out[0] / np.float32(k))
        self.ctl[0] = 0 if j + 1 == k else j + 1
        self.ctl[2] = 0
        self.rng_state[2] = np.uint32((int(self.rng_state[2]) + 1) & 0xFFFFFFFF)
