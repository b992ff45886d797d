"""numpy fp32 restatement of what csrc/optim.hip puts around the Adam arithmetic: the SGD step, AdamW's decay multiply, the clip
coefficient and the group map.  Every operation is one correctly rounded fp32 operation, in the order include/cvx_engine.h gives
(numpy never contracts a multiply and an add).  The Adam core is NOT restated: csrc/optim_core.h (adam_step4 / adam_step1) defines it,
and tests/golden/adam_trace.npz, a trace recorded on the device, pins its bits (tests/test_optim_gpu.py).

tests/test_optim_cpu.py pins these against torch.optim / torch.nn.utils on the CPU; tests/test_optim_gpu.py compares the kernels with them bit for bit."""
import numpy as np

F = np.float32
UNMAPPED = 255


def scaled_grad(g, grad_scale, coef=None):
    """g1 = rn(g * grad_scale); with a clip coefficient g2 = rn(g1 * coef)"""
    x = (np.asarray(g, F) * F(grad_scale)).astype(F)
    if coef is not None:
        x = (x * F(coef)).astype(F)
    return x


def sgd_step(p, b, g2, lr, weight_decay=0.0, momentum=0.0, nesterov=False):
    """torch.optim.SGD, dampening 0 -> (p, b): g3 = rn(g2 + rn(lam*p)); b = rn(rn(mu*b) + g3); d = nesterov ? rn(g3 + rn(mu*b)) : b;
    p = rn(p - rn(lr*d))"""
    p, b, g2 = np.asarray(p, F), np.asarray(b, F), np.asarray(g2, F)
    g3 = (g2 + (F(weight_decay) * p).astype(F)).astype(F)
    b = ((F(momentum) * b).astype(F) + g3).astype(F)
    d = (g3 + (F(momentum) * b).astype(F)).astype(F) if nesterov else b
    p = (p - (F(lr) * d).astype(F)).astype(F)
    return p, b


def decay_factor(lr, weight_decay):
    """fp32 of the double 1 - lr * wd"""
    return F(1.0 - float(lr) * float(weight_decay))


def adamw_decay(p, lr, weight_decay):
    """torch.optim.AdamW's param.mul_(1 - lr * wd)"""
    return (np.asarray(p, F) * decay_factor(lr, weight_decay)).astype(F)


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)), in fp32 from an fp32 norm"""
    den = F(F(norm) + F(1e-6))
    return min(F(1.0), F(F(max_norm) / den))


def build_group_map(n_params, segments):
    """segments: (offset, logical length, group id) -> one uint8 per 16-byte chunk, 255 where nothing lives.  Offsets are multiples of 4;
    the last chunk of a segment whose length is no multiple of 4 belongs to it whole; no chunk has two owners."""
    assert n_params % 4 == 0
    gmap = np.full(n_params // 4, UNMAPPED, np.uint8)
    for off, length, gid in segments:
        assert off % 4 == 0 and length > 0 and 0 <= gid < UNMAPPED
        c0, c1 = off // 4, (off + length + 3) // 4
        assert c1 <= gmap.size and (gmap[c0:c1] == UNMAPPED).all(), "a chunk claimed twice, or a segment behind the arena"
        gmap[c0:c1] = gid
    return gmap
