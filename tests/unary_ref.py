"""Float64 NumPy restatements of bp_unary_forward / bp_unary_backward (include/bp_hip.h, csrc/pointwise.hip): the
saturating layers of the CVAE's layer language.  Views are NHWC arrays (n, h, w, c)."""
import numpy as np

from oracle import ops

KINDS = {"identity": 0, "tanh": 1, "sigmoid": 2, "softplus": 3}
THRESHOLD = 20.0            # torch.nn.Softplus(beta=1, threshold=20): the identity above it


def forward(v, kind):
    """f(v) for the activated input v: 0 identity, 1 tanh, 2 sigmoid, 3 softplus (exactly v above the threshold, as the
    kernel and torch have it; log(1 + e^v) differs from v by less than 2.1e-9 there)."""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == 3:
            return np.where(v > THRESHOLD, v, np.logaddexp(0.0, v))
        return {0: v, 1: np.tanh(v), 2: ops.sigmoid(v)}[kind]


def derivative(y, kind):
    """f' from the saved output y = f(v): 1;  1 - y^2;  y (1 - y);  1 - e^-y (= sigmoid(v), as -expm1(-y))."""
    y = np.asarray(y, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return {0: np.ones_like(y), 1: 1.0 - y * y, 2: y * (1.0 - y), 3: -np.expm1(-y)}[kind]


def backward(dout, dout2, y, kind):
    """d_in = (dout + dout2) * f'(y)."""
    g = np.asarray(dout, np.float64) + (0.0 if dout2 is None else np.asarray(dout2, np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        return g * derivative(y, kind)
