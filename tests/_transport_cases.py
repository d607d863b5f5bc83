"""The case table of test_gpu_transport.py: window counts placed on both sides of every limit at which the library changes how theta
reaches the GPU and how the results come back (launch_forward / enqueue_result_copies in csrc/eincm_api.hip, Engine.loss_grad's staging
buffers).  test_transport_table.py reads the limits from the sources and checks that every one of them is crossed here.

nd = B * h * w * 2: the doubles of theta (and of the gradient) in one evaluation.
"""
from dataclasses import dataclass

H, W, R = 48, 64, 3
DENSE = (H, W)          # theta at the sensor's resolution: the identity scaling, per-pixel flow


@dataclass(frozen=True)
class Case:
    hw: tuple               # theta shape (h, w)
    B: int                  # windows staged
    max_windows: int = 0    # context capacity (0: B); more than B reaches the two-copy result path
    mask: bool = False      # also run a masked evaluation
    tv: bool = False        # gamma > 0 at level 0: the TV term (the Theta image of a 2-DoF theta, k_final)
    tiny: bool = False      # one window of a few events: events * R < 4096 switches the gather's wide variant on
    run_async: bool = False  # also check loss_grad_async / loss_grad_wait against the synchronous call

    @property
    def nd(self):
        return self.B * self.hw[0] * self.hw[1] * 2

    @property
    def cap(self):
        return self.max_windows or self.B

    @property
    def id(self):
        shape = 'dense' if self.hw == DENSE else f'{self.hw[0]}x{self.hw[1]}'
        extra = ''.join(f'-{k}' for k in ('mask', 'tv', 'tiny', 'run_async') if getattr(self, k))
        cap = f'-cap{self.max_windows}' if self.max_windows else ''
        return f'{shape}-B{self.B}{cap}{extra}'


CASES = [
    # 2-DoF: ThetaArg up to 64 windows; 65..2048 the event kernels read the pinned theta buffer while k_theta (TV only) takes
    # ThetaArgBig; from 2049 on theta is read by zero-copy everywhere
    Case((1, 1), 64),
    Case((1, 1), 65, mask=True, run_async=True),
    Case((1, 1), 65, tv=True),
    Case((1, 1), 65, tiny=True),
    Case((1, 1), 2048),
    Case((1, 1), 2049),
    # 4x4: ThetaArg / ThetaArgMid / ThetaArgBig / zero copy; 256 | 257 crosses Engine.loss_grad's cached staging buffers
    Case((4, 4), 4), Case((4, 4), 5),
    Case((4, 4), 16), Case((4, 4), 17),
    Case((4, 4), 128), Case((4, 4), 129),
    Case((4, 4), 256), Case((4, 4), 257),
    # 16x16: ThetaArgMid | ThetaArgBig | zero copy | host-to-device pieces; 128 | 129 also moves the gradient from the gather's
    # host-assembled tail to k_final and a copy back
    Case((16, 16), 1), Case((16, 16), 2),
    Case((16, 16), 8), Case((16, 16), 9),
    Case((16, 16), 128), Case((16, 16), 129, mask=True), Case((16, 16), 129, tiny=True),
    # dense: zero copy | pieces in, one copy | two copies | gradient pieces out
    Case(DENSE, 10), Case(DENSE, 11),
    Case(DENSE, 21), Case(DENSE, 21, max_windows=24),
    Case(DENSE, 22, mask=True, run_async=True),
]
