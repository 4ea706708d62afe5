"""The adaptive controller of DiffAugment's probability restated in numpy float32, in the operation order csrc/ada.hip states
(StyleGAN2-ADA's rule on the sign of the discriminator's real logits): per call

    pend += (sum_b sign(y_b), B)        sign as torch.sign (+-0 -> 0); a logit that is not finite counts 0
    rt_slot += rt_scale * (float32(sum) / float32(B))
    at the iteration's end:  window += pend, pend = 0, steps += 1, and when steps % interval == 0:
        r_t = float32(sign_sum) / float32(count)
        p   = clamp(p + sign(r_t - target) * float32(batch_size * interval) / (kimg * 1000), 0, 1)     all float32, this order
        window = 0
    p_slot = p
"""
import numpy as np

F = np.float32


def signs(y):
    """integer sign sum of the logits y (any float array)"""
    y = np.asarray(y, dtype=np.float32)
    s = np.where(np.isfinite(y), (y > 0).astype(np.int64) - (y < 0).astype(np.int64), 0)
    return int(s.sum())


class Ada:
    def __init__(self, p, target=0.6, interval=4, kimg=500.0, batch_size=1):
        self.p, self.target, self.interval, self.kimg, self.batch_size = F(p), F(target), int(interval), F(kimg), int(batch_size)
        self.sign_sum = self.count = self.steps = 0
        self.pend = [0, 0]

    def state(self):
        return {"p": float(self.p), "sign_sum": self.sign_sum, "count": self.count, "steps": self.steps}

    def add(self, sign_sum, count):
        """one call's integer sums into the iteration's pending pair -> this call's mean sign (float32)"""
        self.pend[0] += int(sign_sum)
        self.pend[1] += int(count)
        return F(sign_sum) / F(count)

    def advance(self):
        """the iteration ends -> p behind it"""
        self.sign_sum += self.pend[0]
        self.count += self.pend[1]
        self.pend = [0, 0]
        self.steps += 1
        if self.steps % self.interval == 0:
            rt = F(self.sign_sum) / F(self.count)
            d = F(rt - self.target)
            sg = F(int(d > 0) - int(d < 0))
            adj = F(F(sg * F(self.batch_size * self.interval)) / F(self.kimg * F(1000.0)))
            self.p = F(min(max(F(self.p + adj), F(0.0)), F(1.0)))
            self.sign_sum = self.count = 0
        return self.p

    def update(self, y):
        """one single-call iteration on logits y -> (this call's mean sign, p) as the kernel's two scalar slots hold them"""
        rt = self.add(signs(y), np.asarray(y).size)
        return rt, self.advance()
