"""Shape helpers used by the map algebra (``pycsou/util/misc.py:15-88``)."""


def is_range_broadcastable(shape1, shape2):
    """Same domain; ranges equal or one of them is 1 (a functional)."""
    if shape1[1] != shape2[1]:
        return False
    return shape1[0] == shape2[0] or shape1[0] == 1 or shape2[0] == 1


def range_broadcast_shape(shape1, shape2):
    if not is_range_broadcastable(shape1, shape2):
        raise ValueError('Shapes are not (range) broadcastable.')
    return (max(shape1[0], shape2[0]), max(shape1[1], shape2[1]))


def peaks(x, y):
    """Matlab's 2-D ``peaks`` surface (``pycsou/util/misc.py:91-127``): translated and scaled Gaussians,

        z = 3 (1 - x)^2 exp(-x^2 - (y + 1)^2) - 10 (x / 5 - x^3 - y^5) exp(-x^2 - y^2)
            - 1/3 exp(-(x + 1)^2 - y^2),

    evaluated on the host at the points given by ``x`` and ``y`` (test signal of the operators' examples)."""
    import numpy as np
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    r2 = x * x + y * y                      # the three Gaussians: centred at (0, -1), (0, 0) and (-1, 0)
    hill = 3.0 * (1.0 - x) ** 2 * np.exp(-(r2 + 2.0 * y + 1.0))
    ridge = 10.0 * (x / 5.0 - x ** 3 - y ** 5) * np.exp(-r2)
    dip = np.exp(-(r2 + 2.0 * x + 1.0)) / 3.0
    return hill - ridge - dip
