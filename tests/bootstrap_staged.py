"""The bootstrap in its staged form, from Evaluator methods that existed before BootstrapPlan: the reference that tests/test_gpu_bootstrap_api.py measures
e_ref with and that tools/bench_bootstrap.py times against.  It needs two levels more than Evaluator::bootstrap: the division by i and the multiplication
by i are multiply_plain by encoded constant vectors, each followed by rescale_to_next (the real half is multiplied by 1 to keep the levels equal).

    mod_raise -> scale := q0 -> coeff_to_slot (c1) -> complex_conjugate, add / sub -> multiply_plain by 1 and by i, rescale_to_next
    -> scale relabel -> two eval_mod calls -> multiply_plain by 1 and by i, rescale_to_next -> add -> slot_to_coeff (c2) -> scale := D

(conj(w) - w = -2i Im w, times i: 2 Im w.)  Every constant is computed from the scales the evaluator tracks: c1 makes EvalMod's working scale the prime it
first divides by, c2 = q0 / (the scale slot_to_coeff will end with)."""
import numpy as np


class Staged:
    def __init__(self, pytroy, ctx, enc, kg, primes, delta, half_width, degree, double_angles, down_layers, up_layers, weight_scale, galois_keys=None):
        """primes: the data primes of the chain (without the special prime).  Builds both slot plans and the Galois keys once."""
        self.pytroy, self.ctx, self.enc, self.primes = pytroy, ctx, enc, [float(p) for p in primes]
        self.delta, self.K, self.degree, self.r, self.W = float(delta), float(half_width), degree, double_angles, float(weight_scale)
        self.slots = enc.slot_count()
        Ld, q = len(primes), self.primes
        gc, gs = len(down_layers), len(up_layers)
        depth = pytroy.chebyshev_depth(degree) + double_angles
        self.levels = gc + 1 + depth + 1 + gs
        assert Ld >= self.levels + 1, "the staged form needs %d data primes" % (self.levels + 1)
        # the scale after coeff_to_slot and the product with the encoded 1 / i (encoded at the prime that rescale_to_next then divides by)
        s = q[0]
        for g in range(gc):
            s = s * self.W / q[Ld - 1 - g]
        L1 = Ld - gc - 1                                           # limbs going into eval_mod
        self.c1 = q[L1 - 1] / (2.0 * self.K * s)                    # the product with 1 / i leaves the scale where it was, up to the prime's rounding
        self.down = pytroy.CoeffToSlotPlan(ctx, enc, ctx.first_parms_id(), self.W, list(down_layers), self.c1)
        self.up_layers = list(up_layers)
        self.constants = {}
        self.up = None                                             # built at the first run, from the scale eval_mod really leaves
        self.gk = galois_keys                                      # given: keys that cover both plans' steps and step 0
        if galois_keys is not None:
            return
        steps = set(self.down.rotation_steps()) | {0}
        # slot_to_coeff's steps do not depend on its constant or level: a plan at the top level names them
        probe = pytroy.SlotToCoeffPlan(ctx, enc, ctx.first_parms_id(), self.W, list(up_layers), 1.0)
        steps |= set(probe.rotation_steps())
        del probe
        self.gk = kg.create_galois_keys_from_steps(sorted(steps), False)

    def _constant(self, ct, value):
        """the constant vector `value` at the level of ct, encoded at the prime that the next rescale divides by"""
        key = (ct.coeff_modulus_size(), complex(value))
        if key not in self.constants:                              # encoded once: a caller would keep them
            prime = self.primes[ct.coeff_modulus_size() - 1]
            self.constants[key] = self.enc.encode_complex64_simd_new([complex(value)] * self.slots, ct.parms_id(), prime)
        return self.constants[key]

    def run(self, ev, rk, exhausted):
        q = self.primes
        raised = ev.mod_raise_new(exhausted)
        raised.set_scale(q[0])
        w = ev.coeff_to_slot_new(raised, self.down, self.gk)
        wbar = ev.complex_conjugate_new(w, self.gk)
        re2 = ev.rescale_to_next_new(ev.multiply_plain_new(ev.add_new(w, wbar), self._constant(w, 1.0)))
        im2 = ev.rescale_to_next_new(ev.multiply_plain_new(ev.sub_new(wbar, w), self._constant(w, 1j)))
        part = re2.scale() * 2.0 * self.c1
        re2.set_scale(part)
        im2.set_scale(part)
        re = ev.eval_mod_new(re2, rk, self.K, self.degree, self.r)
        im = ev.eval_mod_new(im2, rk, self.K, self.degree, self.r)
        re = ev.rescale_to_next_new(ev.multiply_plain_new(re, self._constant(re, 1.0)))
        im = ev.rescale_to_next_new(ev.multiply_plain_new(im, self._constant(im, 1j)))
        y = ev.add_new(re, im)
        if self.up is None:
            s, L = y.scale(), y.coeff_modulus_size()
            for g in range(len(self.up_layers)):
                s = s * self.W / q[L - 1 - g]
            self.up = self.pytroy.SlotToCoeffPlan(self.ctx, self.enc, y.parms_id(), self.W, self.up_layers, q[0] / s)
        out = ev.slot_to_coeff_new(y, self.up, self.gk)
        out.set_scale(self.delta)
        return out


def unit_disc(rng, count):
    z = rng.uniform(-1, 1, count) + 1j * rng.uniform(-1, 1, count)
    return z / np.maximum(np.abs(z), 1.0)
