"""numpy restatement of the trainer's initial state (include/umx_train.h, umx_trainer_init):
``tf.global_variables_initializer()`` of the legacy and the v2 graph as a counter-based stream.

A value is a function of (seed, t = index of the tensor in ``model.tensor_specs`` order, e = flat index inside the tensor):

    key = mix64((seed ^ DOMAIN) + GOLDEN * (t + 1))
    attempt a = 0..15, c = 16 e + a:  u1 = ((mix64(key ^ 2c) >> 11) + 1) 2^-53,  u2 = (mix64(key ^ (2c + 1)) >> 11) 2^-53
    z = sqrt(-2 ln u1) cos(2 pi u2) in float64; the first |z| <= 2 is taken (none: z = 0); value = float32(z * sigma)

BatchNorm tensors hold gamma 1, beta 0, moving mean 0, moving variance 1."""
import numpy as np

from unmicst_amd import model

DOMAIN = np.uint64(0x554D58494E495431)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MAX_ATTEMPTS = 16
TWO_PI = 6.283185307179586
TRUNC_STD = 0.87962566103423978    # standard deviation of a standard normal truncated at +-2


def mix64(x):
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def tensor_key(seed, t):
    with np.errstate(over="ignore"):
        return mix64((np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ DOMAIN) + GOLDEN * np.uint64(t + 1))


def truncated_normal(seed, t, n):
    """n draws z of tensor t, float64: a standard normal redrawn while |z| > 2."""
    key = tensor_key(seed, t)
    z = np.zeros(n, np.float64)
    todo = np.arange(n, dtype=np.uint64)
    for a in range(MAX_ATTEMPTS):
        if todo.size == 0:
            break
        c = todo * np.uint64(MAX_ATTEMPTS) + np.uint64(a)
        two = np.uint64(2)
        u1 = ((mix64(key ^ (two * c)) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
        u2 = (mix64(key ^ (two * c + np.uint64(1))) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        zz = np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)
        ok = np.abs(zz) <= 2.0
        z[todo[ok].astype(np.int64)] = zz[ok]
        todo = todo[~ok]
    return z


def sigma_of(hp, name, shape, std_dev0):
    """None for a BN tensor.  Legacy graph: stdDev0 everywhere.  v2: stdDev0 on ld<i>.w1, else VarianceScaling(scale=1, mode='fan_in')
    as a truncated normal, fan_in = the product of every dimension of the variable's shape but the last."""
    if ".bn." in name:
        return None
    sd0 = float(np.float32(std_dev0))      # the C ABI carries it as a float
    if hp.graph == model.GRAPH_LEGACY or name.endswith(".w1"):
        return sd0
    fan_in = float(np.prod(shape[:-1]))
    return float(np.sqrt(1.0 / fan_in) / TRUNC_STD)


def initial_tensor(seed, t, shape, sigma):
    n = int(np.prod(shape))
    return (truncated_normal(seed, t, n) * sigma).astype(np.float32).reshape(shape)


def initial_tensors(hp, seed, std_dev0):
    out = {}
    for t, (name, shape) in enumerate(model.tensor_specs(hp)):
        sigma = sigma_of(hp, name, shape, std_dev0)
        if sigma is None:
            out[name] = np.full(shape, 1.0 if name.endswith((".gamma", ".var")) else 0.0, np.float32)
        else:
            out[name] = initial_tensor(seed, t, shape, sigma)
    return out


def initial_blob(hp, seed, std_dev0):
    return model.blob_from_tensors(hp, initial_tensors(hp, seed, std_dev0))
