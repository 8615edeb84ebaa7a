"""Host-side handle objects over the C-ABI: Plan (one modulus chain on one GPU) and Behz.

Ciphertext payloads are torch int64 CUDA tensors whose bits are the reference's uint64 words,
layout [batch][poly][limb][N] (ciphertext.h:211-247).  Every method only enqueues work on the
current torch stream; nothing is computed on the CPU.
"""
import ctypes as C
import weakref

import numpy as np
import torch

from . import capi

IDX_COMPONENTWISE, IDX_KS_SET_PRODUCTS, IDX_KS_SKIP_FINALS = 0, 1, 2
ASSIGN_ADD_INPLACE, ASSIGN_OVERWRITE, ASSIGN_OVERWRITE_EXCEPT_FIRST = 0, 1, 2


def to_device(a, device):
    """numpy uint64 array -> int64 CUDA tensor holding the same bits"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_host(t):
    """int64 tensor -> numpy uint64 array (same bits)"""
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _ptr(t):
    if t.dtype != torch.int64 or not t.is_contiguous() or not t.is_cuda:
        raise capi.TroynInvalidArgument("[troyn] operands must be contiguous int64 CUDA tensors")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Plan:
    """troyn_plan: device tables for the key-level modulus chain q_0..q_{K-1} (special prime last).

    Mirrors what ContextData::to_device_inplace (context_data.cu:34-69) uploads for every level.
    """

    def __init__(self, device, log_n, moduli, roots=None):
        self.lib = capi.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise capi.TroynError("[troyn] the hot path runs on an MI355X only; there is no CPU path")
        self.log_n, self.n = int(log_n), 1 << int(log_n)
        self.moduli = [int(q) for q in moduli]
        self.K = len(self.moduli)
        h = C.c_void_p()
        m = (C.c_uint64 * self.K)(*self.moduli)
        r = (C.c_uint64 * self.K)(*[int(x) for x in roots]) if roots is not None else None
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        capi.check(self.lib.troyn_plan_create(C.byref(h), index, self.log_n, self.K, m, r))
        self.h = h
        self._ws = None

    def close(self):
        if getattr(self, "_ckks", None) is not None:
            self._ckks.close()
            self._ckks = None
        if getattr(self, "h", None):
            self.lib.troyn_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ckks_handle(self):
        """the plan's CkksEncoder (troyn_ckks), created on first use"""
        if getattr(self, "_ckks", None) is None:
            self._ckks = CkksEncoder(self)
        return self._ckks

    def set_option(self, name, value=None):
        """an A/B switch of this plan (the library reads the TROYN_* environment variables once, in troyn_plan_create; never on a call)"""
        capi.check(self.lib.troyn_plan_set_option(self.h, name.encode(), None if value is None else str(value).encode()))

    # -- table inspection (known-answer hooks) --------------------------------------------
    def root(self, i):
        out = C.c_uint64()
        capi.check(self.lib.troyn_plan_get_root(self.h, i, C.byref(out)))
        return int(out.value)

    def root_powers(self, i, inverse=False):
        out = np.zeros(2 * self.n, dtype=np.uint64)
        capi.check(self.lib.troyn_plan_get_root_powers(self.h, i, int(inverse), out.ctypes.data_as(capi.p64)))
        return out.reshape(self.n, 2)

    # -- workspace (stands in for the reference's MemoryPool) -------------------------------
    def workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)
        return self._ws

    # -- NTT ---------------------------------------------------------------------------------
    def ntt(self, x, pcount, ncomp, inverse=False, out=None, table_start=0, table_count=None,
            mode=IDX_COMPONENTWISE, decomp=0):
        """x: [batch][pcount][ncomp][N] (any leading shape with that many elements)"""
        if table_count is None:
            table_count = ncomp if mode == IDX_COMPONENTWISE else self.K
        out = x if out is None else out
        batch = x.numel() // (pcount * ncomp * self.n)
        capi.check(self.lib.troyn_ntt(self.h, int(inverse), _ptr(x), _ptr(out), batch, pcount, ncomp,
                                      table_start, table_count, mode, decomp, _stream()))
        return out

    # -- element-wise ---------------------------------------------------------------------------
    def _ew(self, fn, a, b, nmod, mod_start, out):
        out = torch.empty_like(a) if out is None else out
        count = a.numel() // (nmod * self.n)
        if b is None:
            capi.check(fn(self.h, mod_start, nmod, _ptr(a), _ptr(out), count, _stream()))
        else:
            capi.check(fn(self.h, mod_start, nmod, _ptr(a), _ptr(b), _ptr(out), count, _stream()))
        return out

    def add(self, a, b, nmod, mod_start=0, out=None):
        return self._ew(self.lib.troyn_add, a, b, nmod, mod_start, out)

    def sub(self, a, b, nmod, mod_start=0, out=None):
        return self._ew(self.lib.troyn_sub, a, b, nmod, mod_start, out)

    def negate(self, a, nmod, mod_start=0, out=None):
        return self._ew(self.lib.troyn_negate, a, None, nmod, mod_start, out)

    def modulo(self, a, nmod, mod_start=0, out=None):
        """utils::modulo_ps (utils/poly_small_mod.cu:119-180): Barrett-64 reduction of arbitrary 64-bit words"""
        return self._ew(self.lib.troyn_modulo, a, None, nmod, mod_start, out)

    def multiply_uint64operand(self, a, operands, nmod, mod_start=0, out=None):
        """utils::multiply_uint64operand_ps (utils/poly_small_mod.cu:752-814); operands: int64 CUDA tensor [nmod][2] = (operand, quotient)"""
        return self._ew(self.lib.troyn_multiply_uint64operand, a, operands, nmod, mod_start, out)

    def dyadic_product(self, a, b, nmod, mod_start=0, out=None):
        return self._ew(self.lib.troyn_dyadic_product, a, b, nmod, mod_start, out)

    def multiply_scalar(self, a, scalar, nmod, mod_start=0, out=None):
        out = torch.empty_like(a) if out is None else out
        count = a.numel() // (nmod * self.n)
        capi.check(self.lib.troyn_multiply_scalar(self.h, mod_start, nmod, _ptr(a), int(scalar), _ptr(out), count, _stream()))
        return out

    def dyadic_convolute(self, a, pa, b, pb, nmod, mod_start=0, out=None):
        batch = a.numel() // (pa * nmod * self.n)
        if out is None:
            out = torch.empty((batch, pa + pb - 1, nmod, self.n), dtype=torch.int64, device=a.device)
        capi.check(self.lib.troyn_dyadic_convolute(self.h, mod_start, nmod, _ptr(a), pa, _ptr(b), pb, _ptr(out), batch, _stream()))
        return out

    def dyadic_square(self, a, nmod, mod_start=0, out=None):
        batch = a.numel() // (2 * nmod * self.n)
        if out is None:
            out = torch.empty((batch, 3, nmod, self.n), dtype=torch.int64, device=a.device)
        capi.check(self.lib.troyn_dyadic_square(self.h, mod_start, nmod, _ptr(a), _ptr(out), batch, _stream()))
        return out

    # -- ciphertext x plaintext ------------------------------------------------------------------
    def plain_centralize(self, L, t, plain, out=None):
        """plain [batch][N] mod t -> [batch][L][N] (scaling_variant::centralize)"""
        batch = plain.numel() // self.n
        if out is None:
            out = torch.empty((batch, L, self.n), dtype=torch.int64, device=plain.device)
        capi.check(self.lib.troyn_plain_centralize(self.h, L, int(t), _ptr(plain), self.n, self.n, _ptr(out), batch, _stream()))
        return out

    def plain_centralize_ntt(self, L, t, plain, coeff_count=None, out=None):
        """plain [batch][stride] mod t (coeff_count <= stride <= N words used per row) -> NTT form [batch][L][N] in one launch
        (Evaluator::transform_plain_to_ntt = scaling_variant::centralize + forward NTT)"""
        stride = plain.shape[-1]
        batch = plain.numel() // stride
        cc = stride if coeff_count is None else int(coeff_count)
        if out is None:
            out = torch.empty((batch, L, self.n), dtype=torch.int64, device=plain.device)
        capi.check(self.lib.troyn_plain_centralize_ntt(self.h, L, int(t), _ptr(plain), cc, stride, _ptr(out), batch, _stream()))
        return out

    def dyadic_broadcast_product(self, ct, pcount, pt, nmod, shared_plain=False, mod_start=0, out=None):
        """ct [batch][pcount][nmod][N] (.) pt [batch][nmod][N] (or one shared [nmod][N])"""
        batch = ct.numel() // (pcount * nmod * self.n)
        out = torch.empty_like(ct) if out is None else out
        capi.check(self.lib.troyn_dyadic_broadcast_product(self.h, mod_start, nmod, _ptr(ct), pcount, _ptr(pt),
                                                           0 if shared_plain else nmod * self.n, _ptr(out), batch, _stream()))
        return out

    def multiply_plain_accumulate(self, cts, pts, dsts, pcount, nmod, set_zero=True, mod_start=0):
        """dsts[k] (+)= cts[k] (.) pts[k]; equal destination tensors accumulate (multiply_plain_ntt_accumulate)"""
        count = len(cts)
        arr = lambda ts: (C.c_void_p * count)(*[t.data_ptr() for t in ts])
        for t in list(cts) + list(pts) + list(dsts):
            _ptr(t)
        nbytes = self.lib.troyn_multiply_plain_accumulate_workspace_bytes(count)
        ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)
        capi.check(self.lib.troyn_multiply_plain_accumulate(self.h, mod_start, nmod, pcount, arr(cts), arr(pts), arr(dsts), count,
                                                            int(set_zero), C.c_void_p(ws.data_ptr()), ws.numel(), _stream()))
        return dsts

    # -- Galois automorphisms -----------------------------------------------------------------------
    def apply_galois_poly(self, x, nmod, element, is_ntt_form, mod_start=0, out=None):
        """X -> X^element on every polynomial of x [count][nmod][N] (GaloisTool::apply_ps / apply_ntt_ps)"""
        count = x.numel() // (nmod * self.n)
        out = torch.empty_like(x) if out is None else out
        capi.check(self.lib.troyn_apply_galois(self.h, mod_start, nmod, int(is_ntt_form), int(element), _ptr(x), _ptr(out), count, _stream()))
        return out

    def apply_galois_plain(self, x, modulus, element):
        """X -> X^element on coefficient-form polynomials [count][N] modulo one explicit modulus (GaloisTool::apply with the plain modulus)"""
        out = torch.empty_like(x)
        capi.check(self.lib.troyn_apply_galois_plain(self.h, int(modulus), int(element), _ptr(x), _ptr(out), x.numel() // self.n, _stream()))
        return out

    def apply_galois(self, L, ct, element, keys, is_ckks=True, is_ntt_form=True):
        """ct [batch][2][L][N] -> Evaluator::apply_galois: permute both polynomials, key-switch the second"""
        out = self.apply_galois_poly(ct, L, element, is_ntt_form)
        batch = ct.numel() // (2 * L * self.n)
        target = out.view(batch, 2, L, self.n)[:, 1].contiguous()
        self.switch_key(L, target, keys, dest=out.view(batch, 2, L, self.n), assign=ASSIGN_OVERWRITE_EXCEPT_FIRST,
                        is_ckks=is_ckks, is_ntt_form=is_ntt_form)
        return out

    # -- hoisted rotations (additions: one digit decomposition for many Galois keys) ----------------
    def _hoist_entry(self, name, L, is_ckks, is_ntt_form, bgv):
        """(who, function, leading arguments) of a hoisted entry: the plan's own, or its troyn_bgv_* form on a key-level Bgv handle"""
        if bgv is None:
            return "[troyn_%s]" % name, getattr(self.lib, "troyn_" + name), (self.h, L, int(is_ckks), int(is_ntt_form))
        return "[troyn_bgv_%s]" % name, getattr(self.lib, "troyn_bgv_" + name), (bgv.h, L)

    def _apply_galois_hoisted(self, summed, L, ct, elements, keys_per_element, is_ckks, is_ntt_form, out, bgv=None):
        who, fn, head = self._hoist_entry("apply_galois_sum" if summed else "apply_galois_many", L, is_ckks, is_ntt_form, bgv)
        terms = len(elements)
        if len(keys_per_element) != terms:
            raise capi.TroynInvalidArgument("%s one key per Galois element is needed" % who)
        words = 2 * L * self.n
        if L < 1 or ct.numel() % words:
            raise capi.TroynInvalidArgument("%s ct is not [batch][2][L][N]" % who)
        batch = ct.numel() // words
        ptrs = []
        for keys in keys_per_element:
            if len(keys) < L:
                raise capi.TroynInvalidArgument("%s Key switch keys index out of range." % who)
            ptrs += [None if k is None else k.data_ptr() for k in keys[:L]]      # (a null entry is the library's to refuse)
        karr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        earr = (C.c_uint64 * max(terms, 1))(*[int(e) for e in elements])
        shape = (batch, 2, L, self.n) if summed else (terms, batch, 2, L, self.n)
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=self.device)
        elif out.numel() != int(np.prod(shape)):
            raise capi.TroynInvalidArgument("%s out is not %s" % (who, "[batch][2][L][N]" if summed else "[terms][batch][2][L][N]"))
        ws = self.workspace(self.lib.troyn_apply_galois_hoisted_workspace_bytes(self.h, L, terms, batch, int(summed)))
        capi.check(fn(*head, _ptr(ct), earr, karr, terms, _ptr(out), C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    def apply_galois_many(self, L, ct, elements, keys_per_element, is_ckks=True, is_ntt_form=True, out=None):
        """ct [batch][2][L][N] -> [terms][batch][2][L][N]: the key-switched automorphism X -> X^elements[t] of ct for every t, with ONE digit
        decomposition of ct; keys_per_element[t]: the L tensors [2][K][N] of the Galois key of elements[t] (include/troyn.h states the contract)"""
        return self._apply_galois_hoisted(False, L, ct, elements, keys_per_element, is_ckks, is_ntt_form, out)

    def apply_galois_sum(self, L, ct, elements, keys_per_element, is_ckks=True, is_ntt_form=True, out=None):
        """ct [batch][2][L][N] -> [batch][2][L][N]: the SUM over t of the key-switched automorphisms, one decomposition and ONE division by the
        special prime"""
        return self._apply_galois_hoisted(True, L, ct, elements, keys_per_element, is_ckks, is_ntt_form, out)

    def apply_galois_weighted_sums(self, L, ct, elements, keys_per_element, weights, is_ckks=True, is_ntt_form=True, out=None):
        """ct [batch][2][L][N] -> [slots][batch][2][L][N]: out[s] = SUM_t weights[s][t] (.) (key-switched automorphism X -> X^elements[t] of ct),
        one digit decomposition and ONE division by the special prime per slot (the diagonal method; include/troyn.h states the contract).
        weights[s][t]: a tensor [K][N] in NTT form and key-level layout (special prime last), or None = the term is absent from slot s.
        The element 1 is the unrotated ciphertext; its entry of keys_per_element may be None."""
        return self._apply_galois_weighted_sums(L, ct, elements, keys_per_element, weights, is_ckks, is_ntt_form, out)

    def _apply_galois_weighted_sums(self, L, ct, elements, keys_per_element, weights, is_ckks, is_ntt_form, out, bgv=None):
        who, fn, head = self._hoist_entry("apply_galois_weighted_sums", L, is_ckks, is_ntt_form, bgv)
        terms, slots = len(elements), len(weights)
        if len(keys_per_element) != terms:
            raise capi.TroynInvalidArgument("%s one key per Galois element is needed" % who)
        words = 2 * L * self.n
        if L < 1 or ct.numel() % words:
            raise capi.TroynInvalidArgument("%s ct is not [batch][2][L][N]" % who)
        batch = ct.numel() // words
        ptrs = []
        for e, keys in zip(elements, keys_per_element):
            if keys is None and int(e) == 1:
                keys = [None] * L
            if keys is None or len(keys) < L:
                raise capi.TroynInvalidArgument("%s Key switch keys index out of range." % who)
            ptrs += [None if k is None else k.data_ptr() for k in keys[:L]]      # (a null entry is the library's to refuse)
        wptrs = []
        for row in weights:
            if len(row) != terms:
                raise capi.TroynInvalidArgument("%s one weight (or None) per slot and term is needed" % who)
            for w in row:
                if w is not None and w.numel() != self.K * self.n:
                    raise capi.TroynInvalidArgument("%s a weight is not [K][N]" % who)
                wptrs.append(None if w is None else w.data_ptr())
        karr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        warr = (C.c_void_p * max(len(wptrs), 1))(*wptrs)
        earr = (C.c_uint64 * max(terms, 1))(*[int(e) for e in elements])
        shape = (slots, batch, 2, L, self.n)
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=self.device)
        elif out.numel() != int(np.prod(shape)):
            raise capi.TroynInvalidArgument("%s out is not [slots][batch][2][L][N]" % who)
        ws = self.workspace(self.lib.troyn_apply_galois_weighted_workspace_bytes(self.h, L, terms, slots, batch, int(is_ntt_form)))
        capi.check(fn(*head, _ptr(ct), earr, karr, terms, warr, slots, _ptr(out), C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    # -- sums over different ciphertexts and the baby-step/giant-step transform (additions) ---------
    def _keyed_tables(self, who, L, elements, keys_per_element):
        """the element and key-pointer tables of one stage; the entry of the element 1 may be None"""
        if len(keys_per_element) != len(elements):
            raise capi.TroynInvalidArgument("%s one key per Galois element is needed" % who)
        ptrs = []
        for e, keys in zip(elements, keys_per_element):
            if keys is None and int(e) == 1:
                keys = [None] * L
            if keys is None or len(keys) < L:
                raise capi.TroynInvalidArgument("%s Key switch keys index out of range." % who)
            ptrs += [None if k is None else k.data_ptr() for k in keys[:L]]      # (a null entry is the library's to refuse)
        karr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        earr = (C.c_uint64 * max(len(elements), 1))(*[int(e) for e in elements])
        return earr, karr

    def apply_galois_sum_each(self, L, cts, elements, keys_per_element, is_ckks=True, is_ntt_form=True, out=None):
        """cts [terms][batch][2][L][N] -> [batch][2][L][N]: the SUM over t of the key-switched automorphism X -> X^elements[t] of cts[t], one
        ciphertext PER TERM, summed before ONE division by the special prime (include/troyn.h states the contract).  The element 1 adds the
        term unrotated; its entry of keys_per_element may be None."""
        return self._apply_galois_sum_each(L, cts, elements, keys_per_element, is_ckks, is_ntt_form, out)

    def _apply_galois_sum_each(self, L, cts, elements, keys_per_element, is_ckks, is_ntt_form, out, bgv=None):
        who, fn, head = self._hoist_entry("apply_galois_sum_each", L, is_ckks, is_ntt_form, bgv)
        terms = len(elements)
        earr, karr = self._keyed_tables(who, L, elements, keys_per_element)
        words = 2 * L * self.n
        if terms == 0:
            raise capi.TroynInvalidArgument("%s no terms" % who)
        if L < 1 or cts.numel() % (terms * words):
            raise capi.TroynInvalidArgument("%s cts is not [terms][batch][2][L][N]" % who)
        batch = cts.numel() // (terms * words)
        shape = (batch, 2, L, self.n)
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=self.device)
        elif out.numel() != int(np.prod(shape)):
            raise capi.TroynInvalidArgument("%s out is not [batch][2][L][N]" % who)
        ws = self.workspace(self.lib.troyn_apply_galois_sum_each_workspace_bytes(self.h, L, terms, batch, int(is_ntt_form)))
        capi.check(fn(*head, _ptr(cts), earr, karr, terms, _ptr(out), C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    def linear_transform_bsgs(self, L, ct, baby_elements, baby_keys, giant_elements, giant_keys, weights, is_ckks=True, is_ntt_form=True,
                              out=None):
        """ct [batch][2][L][N] -> [batch][2][L][N]: SUM_g sigma_G[g]( SUM_b weights[g][b] (.) sigma_B[b](ct) ), the baby-step/giant-step form of
        a plaintext matrix times an encrypted vector: one digit decomposition of ct, one division per giant step for the inner sums and ONE
        for the outer sum.  weights[g][b]: a tensor [K][N] in NTT form and key-level layout, ALREADY rotated back by the giant step, or None;
        every giant step needs a weight.  The element 1 is the identity in either list; its keys may be None."""
        return self._linear_transform_bsgs("troyn_linear_transform_bsgs", L, ct, baby_elements, baby_keys, giant_elements, giant_keys, weights,
                                           is_ckks, is_ntt_form, out)

    def linear_transform_bsgs_double_hoisted(self, L, ct, baby_elements, baby_keys, giant_elements, giant_keys, weights, is_ckks=True,
                                             is_ntt_form=True, out=None):
        """linear_transform_bsgs with the second hoisting level: the inner sums stay on the extended basis, only component 1 of a giant step
        with a key is divided, and ONE division ends the transform.  Same arguments; the words differ from linear_transform_bsgs (one
        rounding per giant step fewer), the decrypted message does not."""
        return self._linear_transform_bsgs("troyn_linear_transform_bsgs_double_hoisted", L, ct, baby_elements, baby_keys, giant_elements,
                                           giant_keys, weights, is_ckks, is_ntt_form, out)

    def _linear_transform_bsgs(self, entry, L, ct, baby_elements, baby_keys, giant_elements, giant_keys, weights, is_ckks, is_ntt_form, out,
                               bgv=None):
        who, fn, head = self._hoist_entry(entry[len("troyn_"):], L, is_ckks, is_ntt_form, bgv)
        babies, giants = len(baby_elements), len(giant_elements)
        bearr, bkarr = self._keyed_tables(who, L, baby_elements, baby_keys)
        gearr, gkarr = self._keyed_tables(who, L, giant_elements, giant_keys)
        words = 2 * L * self.n
        if L < 1 or ct.numel() % words:
            raise capi.TroynInvalidArgument("%s ct is not [batch][2][L][N]" % who)
        batch = ct.numel() // words
        if len(weights) != giants:
            raise capi.TroynInvalidArgument("%s one weight row per giant step is needed" % who)
        wptrs = []
        for row in weights:
            if len(row) != babies:
                raise capi.TroynInvalidArgument("%s one weight (or None) per giant and baby step is needed" % who)
            for w in row:
                if w is not None and w.numel() != self.K * self.n:
                    raise capi.TroynInvalidArgument("%s a weight is not [K][N]" % who)
                wptrs.append(None if w is None else w.data_ptr())
        warr = (C.c_void_p * max(len(wptrs), 1))(*wptrs)
        shape = (batch, 2, L, self.n)
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=self.device)
        elif out.numel() != int(np.prod(shape)):
            raise capi.TroynInvalidArgument("%s out is not [batch][2][L][N]" % who)
        ws = self.workspace(getattr(self.lib, entry + "_workspace_bytes")(self.h, L, babies, giants, batch, int(is_ntt_form)))
        capi.check(fn(*head, _ptr(ct), bearr, bkarr, babies, gearr, gkarr, giants, warr, _ptr(out),
                      C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    # -- RLWE / LWE packing (evaluator_lwes.cu) -----------------------------------------------------
    def negacyclic_shift(self, x, nmod, shift, mod_start=0):
        """x [count][nmod][N] * X^shift (utils::negacyclic_shift_ps), any shift (modulo 2N)"""
        out = torch.empty_like(x)
        capi.check(self.lib.troyn_negacyclic_shift(self.h, mod_start, nmod, _ptr(x), _ptr(out), int(shift), x.numel() // (nmod * self.n), _stream()))
        return out

    def multiply_inv_degree(self, x, nmod, scalar, mod_start=0, out=None):
        """x * N^-1 * scalar (utils::ntt_multiply_inv_degree); in place when out is x"""
        out = torch.empty_like(x) if out is None else out
        capi.check(self.lib.troyn_multiply_inv_degree(self.h, mod_start, nmod, _ptr(x), _ptr(out), int(scalar), x.numel() // (nmod * self.n), _stream()))
        return out

    def extract_lwe(self, L, cts, terms):
        """Evaluator::extract_lwe_new for (cts[i], terms[i]); cts: coefficient-form tensors [2][L][N] -> c0 [count][L], c1 [count][L][N]"""
        count = len(cts)
        c0 = torch.empty((count, L), dtype=torch.int64, device=self.device)
        c1 = torch.empty((count, L, self.n), dtype=torch.int64, device=self.device)
        ptrs = (C.c_void_p * count)(*[c.data_ptr() for c in cts])
        tarr = (C.c_size_t * count)(*[int(t) for t in terms])
        ws = self.workspace(self.lib.troyn_extract_lwe_workspace_bytes(count))
        capi.check(self.lib.troyn_extract_lwe(self.h, L, ptrs, tarr, _ptr(c0), _ptr(c1), count, C.c_void_p(ws.data_ptr()), ws.numel(), _stream()))
        return c0, c1

    def pack_rlwe_ciphertexts(self, L, groups, keys_by_element, shift, input_interval, output_interval, is_ckks=False, apply_field_trace=True):
        """Evaluator::pack_rlwe_ciphertexts_new_batched (evaluator_lwes.cu:491-681) for coefficient-form two-polynomial
        ciphertexts: groups = list of lists of tensors [2][L][N]; returns [len(groups)][2][L][N] (coefficient form).
        One working buffer holds every group's slots in bit-reversed order; each layer is troyn_pack_layer + one batched
        troyn_switch_key and halves the buffer."""
        n, G = self.n, len(groups)
        maxc = input_interval // output_interval
        layers = maxc.bit_length() - 1
        slots = G * maxc
        src = (C.c_void_p * slots)()
        for g, cts in enumerate(groups):
            if not 1 <= len(cts) <= maxc:
                raise capi.TroynInvalidArgument("[Evaluator::pack_rlwe_ciphertexts_new] ciphers count must be less than input_interval / output_interval.")
            for i in range(maxc):
                index = int("{:0{w}b}".format(i, w=layers)[::-1], 2) if layers else 0
                src[g * maxc + i] = cts[index].data_ptr() if index < len(cts) else None
        cur = torch.empty((slots, 2, L, n), dtype=torch.int64, device=self.device)
        ws = self.workspace(self.lib.troyn_pack_prepare_workspace_bytes(slots))
        capi.check(self.lib.troyn_pack_prepare(self.h, L, 2, src, slots, n // input_interval, int(shift), _ptr(cur),
                                               C.c_void_p(ws.data_ptr()), ws.numel(), _stream()))
        for layer in range(layers):
            pairs = cur.shape[0] // 2
            g = (n // input_interval) * (1 << (layer + 1)) + 1
            nxt = torch.empty((pairs, 2, L, n), dtype=torch.int64, device=self.device)
            target = torch.empty((pairs, L, n), dtype=torch.int64, device=self.device)
            capi.check(self.lib.troyn_pack_layer(self.h, L, g, input_interval >> (layer + 1), _ptr(cur), _ptr(nxt), _ptr(target), pairs, _stream()))
            self.switch_key(L, target, keys_by_element[g], dest=nxt, assign=ASSIGN_ADD_INPLACE, is_ckks=is_ckks, is_ntt_form=False)
            cur = nxt
        if output_interval != 1 and apply_field_trace:
            d = n
            while d > n // output_interval:
                cur = self.add(cur, self.apply_galois(L, cur, d + 1, keys_by_element[d + 1], is_ckks=is_ckks, is_ntt_form=False), L)
                d >>= 1
        return cur

    # -- key switching -----------------------------------------------------------------------------
    def _key_ptrs(self, keys, L):
        if len(keys) < L:
            raise capi.TroynInvalidArgument("[Evaluator::switch_key_inplace_internal] Key switch keys index out of range.")
        arr = (C.c_void_p * L)(*[k.data_ptr() for k in keys[:L]])
        return arr

    def switch_key(self, L, target, keys, dest=None, assign=ASSIGN_OVERWRITE, is_ckks=True, is_ntt_form=True):
        """target [batch][L][N]; keys: list of L tensors [2][K][N]; dest [batch][2][L][N]"""
        batch = target.numel() // (L * self.n)
        if dest is None:
            dest = torch.zeros((batch, 2, L, self.n), dtype=torch.int64, device=target.device)
        nbytes = self.lib.troyn_switch_key_workspace_bytes(self.h, L, batch)
        ws = self.workspace(nbytes)
        capi.check(self.lib.troyn_switch_key(self.h, L, int(is_ckks), int(is_ntt_form), _ptr(target), self._key_ptrs(keys, L),
                                             assign, _ptr(dest), C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return dest

    def relinearize(self, L, ct3, keys, out=None, is_ckks=True, is_ntt_form=True):
        """ct3 [batch][3][L][N] -> [batch][2][L][N]"""
        batch = ct3.numel() // (3 * L * self.n)
        if out is None:
            out = torch.empty((batch, 2, L, self.n), dtype=torch.int64, device=ct3.device)
        nbytes = self.lib.troyn_relinearize_workspace_bytes(self.h, L, batch)
        ws = self.workspace(nbytes)
        capi.check(self.lib.troyn_relinearize(self.h, L, int(is_ckks), int(is_ntt_form), _ptr(ct3), self._key_ptrs(keys, L),
                                              _ptr(out), C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    def ckks_multiply_relinearize_rescale(self, L, a, b, keys, out=None):
        """a, b [batch][2][L][N] (NTT form) -> rescale_to_next(relinearize(multiply(a, b))) [batch][2][L-1][N], one call"""
        batch = a.numel() // (2 * L * self.n)
        if out is None:
            out = torch.empty((batch, 2, L - 1, self.n), dtype=torch.int64, device=a.device)
        nbytes = self.lib.troyn_ckks_multiply_relinearize_rescale_workspace_bytes(self.h, L, batch)
        ws = self.workspace(nbytes)
        capi.check(self.lib.troyn_ckks_multiply_relinearize_rescale(self.h, L, _ptr(a), _ptr(b), self._key_ptrs(keys, L), _ptr(out),
                                                                    C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    # -- dot products of ciphertexts (additions: lazy relinearization) -----------------------------------
    def _term_ptrs(self, who, a_list, b_list, words_per_item):
        """two lists of [batch][2][nmod][N] tensors (None stands for a null entry) -> (two host arrays of device pointers, batch); every tensor of
        both lists must hold the same number of words: the kernel reads `batch` items behind every pointer"""
        if len(a_list) != len(b_list):
            raise capi.TroynInvalidArgument("%s the two lists have different lengths" % who)
        sizes = set()
        for t in list(a_list) + list(b_list):
            if t is not None:
                _ptr(t)
                sizes.add(t.numel())
        if len(sizes) > 1:
            raise capi.TroynInvalidArgument("%s operands of different sizes" % who)
        words = sizes.pop() if sizes else 0
        if words_per_item and words % words_per_item:
            raise capi.TroynInvalidArgument("%s operands are not [batch][2][nmod][N]" % who)
        arr = lambda ts: (C.c_void_p * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])
        return arr(a_list), arr(b_list), (words // words_per_item if words_per_item else 0)      # (an empty slice is the library's to refuse)

    def dyadic_convolute_accumulate(self, a_list, b_list, nmod, mod_start=0, out=None, accumulate=False):
        """out [batch][3][nmod][N] (+)= SUM_t a_list[t] (x) b_list[t], every operand [batch][2][nmod][N] in NTT form; one pass over the terms"""
        who = "[troyn_dyadic_convolute_accumulate]"
        pa, pb, batch = self._term_ptrs(who, a_list, b_list, 2 * nmod * self.n)
        if out is None:
            if accumulate:
                raise capi.TroynInvalidArgument("%s accumulate needs an out tensor" % who)
            out = torch.empty((batch, 3, nmod, self.n), dtype=torch.int64, device=self.device)
        elif out.numel() != batch * 3 * nmod * self.n:
            raise capi.TroynInvalidArgument("%s out is not [batch][3][nmod][N]" % who)
        capi.check(self.lib.troyn_dyadic_convolute_accumulate(self.h, mod_start, nmod, pa, pb, len(a_list), _ptr(out), int(bool(accumulate)), batch, _stream()))
        return out

    def ckks_multiply_accumulate_relinearize_rescale(self, L, a_list, b_list, keys, out=None):
        """rescale_to_next(relinearize(SUM_t multiply(a_list[t], b_list[t]))) -> [batch][2][L-1][N]: one key switch and one rescale for the sum"""
        who = "[troyn_ckks_multiply_accumulate_relinearize_rescale]"
        pa, pb, batch = self._term_ptrs(who, a_list, b_list, 2 * L * self.n)
        if out is None:
            out = torch.empty((batch, 2, max(L - 1, 0), self.n), dtype=torch.int64, device=self.device)
        elif out.numel() != batch * 2 * (L - 1) * self.n:
            raise capi.TroynInvalidArgument("%s out is not [batch][2][L-1][N]" % who)
        nbytes = self.lib.troyn_ckks_multiply_accumulate_relinearize_rescale_workspace_bytes(self.h, L, len(a_list), batch)
        ws = self.workspace(nbytes)
        capi.check(self.lib.troyn_ckks_multiply_accumulate_relinearize_rescale(self.h, L, pa, pb, len(a_list), self._key_ptrs(keys, L), _ptr(out),
                                                                               C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    def scalar_weighted_sums(self, inputs, in_nmod, scalars, nmod, pcount, constants=None, constant_at_index0=False, mod_start=0, out=None, batch=None):
        """out [slots][batch][pcount][nmod][N]: out[s] = SUM_t scalars[s][t] * inputs[t] (+ constants[s] on polynomial 0), one pass over the inputs
        for every tile of slots (include/troyn.h states the contract).  inputs[t]: [batch][pcount][in_nmod[t]][N] with in_nmod[t] >= nmod, only
        its first nmod limbs are read; scalars [slots][terms][nmod] and constants [slots][nmod] (or None) are canonical residues on the host.
        `batch` is taken from inputs[0] unless given (batch = 0 launches nothing and looks at no buffer: entries and `out` may be None)."""
        who = "[troyn_scalar_weighted_sums]"
        terms = len(inputs)
        if len(in_nmod) != terms:
            raise capi.TroynInvalidArgument("%s one limb count per input is needed" % who)
        sc = np.ascontiguousarray(np.array(scalars, dtype=np.uint64))
        slots = len(scalars)
        if terms and slots and nmod and sc.shape != (slots, terms, nmod):      # (an empty table is the library's to refuse)
            raise capi.TroynInvalidArgument("%s scalars are not [slots][terms][nmod]" % who)
        if sc.size == 0:
            sc = np.zeros(1, dtype=np.uint64)
        cs = None
        if constants is not None:
            cs = np.ascontiguousarray(np.array(constants, dtype=np.uint64))
            if cs.shape != (slots, nmod):
                raise capi.TroynInvalidArgument("%s constants are not [slots][nmod]" % who)
        if batch is None:
            words = pcount * int(in_nmod[0]) * self.n if terms else 0
            if not words or inputs[0] is None or inputs[0].numel() % words:
                raise capi.TroynInvalidArgument("%s inputs[0] is not [batch][pcount][in_nmod[0]][N]" % who)
            batch = inputs[0].numel() // words
        for t, x in enumerate(inputs):
            if x is not None and batch and x.numel() != batch * pcount * int(in_nmod[t]) * self.n:
                raise capi.TroynInvalidArgument("%s inputs[%d] is not [batch][pcount][in_nmod][N]" % (who, t))
        parr = (C.c_void_p * max(terms, 1))(*[None if x is None else _ptr(x).value for x in inputs])
        narr = (C.c_uint32 * max(terms, 1))(*[int(v) for v in in_nmod])
        shape = (slots, batch, pcount, nmod, self.n)
        if out is None and batch:
            out = torch.empty(shape, dtype=torch.int64, device=self.device)
        elif out is not None and out.numel() != int(np.prod(shape)):
            raise capi.TroynInvalidArgument("%s out is not [slots][batch][pcount][nmod][N]" % who)
        ws = self.workspace(self.lib.troyn_scalar_weighted_sums_workspace_bytes(self.h, nmod, terms, slots)) if batch else None
        capi.check(self.lib.troyn_scalar_weighted_sums(
            self.h, mod_start, nmod, parr, narr, terms, sc.ctypes.data_as(capi.p64), None if cs is None else cs.ctypes.data_as(capi.p64),
            int(bool(constant_at_index0)), pcount, None if out is None else _ptr(out), slots, batch,
            None if ws is None else C.c_void_p(ws.data_ptr()), 0 if ws is None else ws.numel(), _stream()))
        return out

    def multiply_affine_relinearize_rescale(self, L, a_list, b_list, c_list, c_nmod, alpha, weight, keys, constant=None, out=None):
        """out [batch][2][L-1][N]: out[i] = rescale_to_next(relinearize(alpha[i] * a_list[i] (x) b_list[i] + weight[i] * c_list[i] + constant[i])), the
        Chebyshev recurrence / double angle as one step (include/troyn.h states the contract).  a_list[i], b_list[i]: [2][L][N]; c_list[i]:
        [2][c_nmod[i]][N] with c_nmod[i] >= L, or None (no addend; c_list itself may be None); alpha, weight [batch][L] and constant [batch][L] (or None) are canonical
        residues on the host.  An empty batch launches nothing and looks at no buffer."""
        who = "[troyn_ckks_multiply_affine_relinearize_rescale]"
        batch = len(a_list)
        if c_list is None:      # no addend anywhere (the double angle): c_nmod and weight may be None as well
            c_list, c_nmod = [None] * batch, [0] * batch
            weight = [[0] * L] * batch if weight is None else weight
        if len(b_list) != batch or len(c_list) != batch or len(c_nmod) != batch:
            raise capi.TroynInvalidArgument("%s one b, c and limb count per item is needed" % who)
        tabs = []
        for name, t in (("alpha", alpha), ("weight", weight), ("constant", constant)):
            if t is None and name == "constant":
                tabs.append(None)
                continue
            arr = np.ascontiguousarray(np.array(t, dtype=np.uint64))
            if batch and arr.shape != (batch, L):
                raise capi.TroynInvalidArgument("%s %s is not [batch][L]" % (who, name))
            tabs.append(arr if arr.size else np.zeros(1, dtype=np.uint64))
        for name, ts, words in (("a", a_list, [2 * L * self.n] * batch), ("b", b_list, [2 * L * self.n] * batch),
                                ("c", c_list, [2 * int(v) * self.n for v in c_nmod])):
            for i, t in enumerate(ts):
                if t is not None and _ptr(t) and t.numel() != words[i]:
                    raise capi.TroynInvalidArgument("%s %s[%d] is not [2][limbs][N]" % (who, name, i))
        arr = lambda ts: (C.c_void_p * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])
        narr = (C.c_uint32 * max(batch, 1))(*[int(v) for v in c_nmod])
        if out is None and batch:
            out = torch.empty((batch, 2, max(L - 1, 0), self.n), dtype=torch.int64, device=self.device)
        elif out is not None and out.numel() != batch * 2 * (L - 1) * self.n:
            raise capi.TroynInvalidArgument("%s out is not [batch][2][L-1][N]" % who)
        ws = self.workspace(self.lib.troyn_ckks_multiply_affine_relinearize_rescale_workspace_bytes(self.h, L, batch)) if batch else None
        capi.check(self.lib.troyn_ckks_multiply_affine_relinearize_rescale(
            self.h, L, arr(a_list), arr(b_list), arr(c_list), narr, tabs[0].ctypes.data_as(capi.p64), tabs[1].ctypes.data_as(capi.p64),
            None if tabs[2] is None else tabs[2].ctypes.data_as(capi.p64), self._key_ptrs(keys, L) if batch else None,
            None if out is None else _ptr(out), None if ws is None else C.c_void_p(ws.data_ptr()), 0 if ws is None else ws.numel(), batch, _stream()))
        return out

    def ckks_complex_split(self, L, a, b, s=None, d=None):
        """troyn_ckks_complex_split: a, b [batch][2][L][N] in NTT form (a ciphertext and its complex conjugate) -> (s, d) = (a + b, mu . (b - a)), mu the
        forward transform of X^(N/2): slots 2 Re and (-1)^j 2 Im, no level spent (include/troyn.h states the contract)"""
        batch = a.numel() // (2 * L * self.n) if L else 0
        s = torch.empty_like(a) if s is None else s
        d = torch.empty_like(a) if d is None else d
        capi.check(self.lib.troyn_ckks_complex_split(self.h, L, _ptr(a), _ptr(b), _ptr(s), _ptr(d), batch, _stream()))
        return s, d

    def ckks_complex_join(self, L, a, b, out=None):
        """troyn_ckks_complex_join: out = a + mu . b on [batch][2][L][N] in NTT form: slots Re + i Im from slots Re and (-1)^j Im"""
        batch = a.numel() // (2 * L * self.n) if L else 0
        out = torch.empty_like(a) if out is None else out
        capi.check(self.lib.troyn_ckks_complex_join(self.h, L, _ptr(a), _ptr(b), _ptr(out), batch, _stream()))
        return out

    # -- modulus switching -------------------------------------------------------------------------
    def divide_and_round_q_last(self, L, x, pcount, out=None):
        batch = x.numel() // (pcount * L * self.n)
        if out is None:
            out = torch.empty((batch, pcount, L - 1, self.n), dtype=torch.int64, device=x.device)
        capi.check(self.lib.troyn_divide_and_round_q_last(self.h, L, _ptr(x), pcount, _ptr(out), batch, _stream()))
        return out

    def divide_and_round_q_last_ntt(self, L, x, pcount, out=None):
        batch = x.numel() // (pcount * L * self.n)
        if out is None:
            out = torch.empty((batch, pcount, L - 1, self.n), dtype=torch.int64, device=x.device)
        nbytes = self.lib.troyn_divide_and_round_q_last_ntt_workspace_bytes(self.h, L, pcount, batch)
        ws = self.workspace(nbytes)
        capi.check(self.lib.troyn_divide_and_round_q_last_ntt(self.h, L, _ptr(x), pcount, _ptr(out),
                                                              C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    def mod_switch_drop(self, L_in, L_out, x, pcount, out=None):
        batch = x.numel() // (pcount * L_in * self.n)
        if out is None:
            out = torch.empty((batch, pcount, L_out, self.n), dtype=torch.int64, device=x.device)
        capi.check(self.lib.troyn_mod_switch_drop(self.h, L_in, L_out, _ptr(x), pcount, _ptr(out), batch, _stream()))
        return out


class Prng:
    """The context generator (AES-128-CTR, utils/random_generator.cu): seed + block counter on the host, sampling
    kernels on the device."""

    def __init__(self, plan, seed_low, seed_high=0):
        self.plan = plan
        self.seed = np.array([seed_low, seed_high], dtype=np.uint64)
        self.counter = 0

    def sample_uint64(self):
        out = np.zeros(2, dtype=np.uint64)
        capi.check(self.plan.lib.troyn_prng_block(self.seed.ctypes.data_as(capi.p64), self.counter, out.ctypes.data_as(capi.p64)))
        self.counter += 1
        return int(out[0])

    def _sample(self, fn, nmod):
        out = torch.empty((nmod, self.plan.n), dtype=torch.int64, device=self.plan.device)
        used = np.zeros(1, dtype=np.uint64)
        capi.check(getattr(self.plan.lib, fn)(self.plan.h, nmod, self.seed.ctypes.data_as(capi.p64), self.counter, _ptr(out),
                                              used.ctypes.data_as(capi.p64), _stream()))
        self.counter += int(used[0])
        return out

    def ternary(self, nmod):
        return self._sample("troyn_sample_ternary", nmod)

    def ternary_sparse(self, nmod, h):
        """A ternary polynomial with exactly `h` nonzero coefficients (troyn_sample_ternary_sparse: the h smallest of N keyed words)."""
        out = torch.empty((nmod, self.plan.n), dtype=torch.int64, device=self.plan.device)
        used = np.zeros(1, dtype=np.uint64)
        capi.check(self.plan.lib.troyn_sample_ternary_sparse(self.plan.h, nmod, self.seed.ctypes.data_as(capi.p64), self.counter, int(h), _ptr(out),
                                                             used.ctypes.data_as(capi.p64), _stream()))
        self.counter += int(used[0])
        return out

    def centered_binomial(self, nmod):
        return self._sample("troyn_sample_centered_binomial", nmod)

    def uniform(self, nmod):
        return self._sample("troyn_sample_uniform", nmod)

    def centered_binomial_strided(self, nmod, count, counter_stride):
        """`count` noise polynomials; item i reads the blocks from counter + i*counter_stride (the positions `count`
        sequential encryptions would use).  The counter is not advanced: the caller owns the block range."""
        out = torch.empty((count, nmod, self.plan.n), dtype=torch.int64, device=self.plan.device)
        capi.check(self.plan.lib.troyn_sample_centered_binomial_strided(self.plan.h, nmod, self.seed.ctypes.data_as(capi.p64), self.counter,
                                                                        int(counter_stride), _ptr(out), count, _stream()))
        return out


def sample_uniform_multi(plan, nmod, seeds):
    """One uniform RNS polynomial per seed pair (low, high), each from block 0 of its own generator (the c1 generators
    of `len(seeds)` symmetric encryptions, utils/rlwe.cu:252-262)."""
    sd = np.ascontiguousarray(np.array(seeds, dtype=np.uint64).reshape(-1, 2))
    out = torch.empty((sd.shape[0], nmod, plan.n), dtype=torch.int64, device=plan.device)
    capi.check(plan.lib.troyn_sample_uniform_multi(plan.h, nmod, sd.ctypes.data_as(capi.p64), _ptr(out), sd.shape[0], _stream()))
    return out


class Bgv:
    """troyn_bgv: the BGV-only constants of one level (RNSTool, utils/rns_tool.cu:205-232) and the steps that use them."""

    def __init__(self, plan, L, plain_modulus):
        self.plan, self.L, self.t = plan, int(L), int(plain_modulus)
        h = C.c_void_p()
        capi.check(plan.lib.troyn_bgv_create(C.byref(h), plan.h, self.L, self.t))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.plan.lib.troyn_bgv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def inv_q_last_mod_t(self):
        return int(self.plan.lib.troyn_bgv_inv_q_last_mod_t(self.h))

    def mod_t_and_divide_q_last_ntt(self, x, pcount, out=None):
        """x [batch][pcount][L][N] NTT form -> [batch][pcount][L-1][N]"""
        n, L = self.plan.n, self.L
        batch = x.numel() // (pcount * L * n)
        if out is None:
            out = torch.empty((batch, pcount, L - 1, n), dtype=torch.int64, device=x.device)
        ws = self.plan.workspace(self.plan.lib.troyn_bgv_mod_switch_workspace_bytes(self.h, pcount, batch))
        capi.check(self.plan.lib.troyn_bgv_mod_t_and_divide_q_last_ntt(self.h, _ptr(x), pcount, _ptr(out), C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    def decrypt_mod_t(self, phase, correction_factor=1):
        """phase [batch][L][N] coefficient form -> [batch][N] mod t (times correction_factor^-1)"""
        n = self.plan.n
        batch = phase.numel() // (self.L * n)
        out = torch.empty((batch, n), dtype=torch.int64, device=phase.device)
        capi.check(self.plan.lib.troyn_bgv_decrypt_mod_t(self.h, _ptr(phase), int(correction_factor), _ptr(out), batch, _stream()))
        return out

    def multiply_scalar_mod_t(self, x, scalar):
        out = torch.empty_like(x)
        capi.check(self.plan.lib.troyn_bgv_multiply_scalar_mod_t(self.h, _ptr(x), int(scalar), _ptr(out), x.numel(), _stream()))
        return out

    def switch_key(self, L, target, keys, dest=None, assign=ASSIGN_OVERWRITE):
        """self must be the key level (L = plan.K); target [batch][L][N] NTT form"""
        plan = self.plan
        batch = target.numel() // (L * plan.n)
        if dest is None:
            dest = torch.zeros((batch, 2, L, plan.n), dtype=torch.int64, device=target.device)
        ws = plan.workspace(plan.lib.troyn_switch_key_workspace_bytes(plan.h, L, batch))
        capi.check(plan.lib.troyn_bgv_switch_key(self.h, L, _ptr(target), plan._key_ptrs(keys, L), assign, _ptr(dest), C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return dest

    def relinearize(self, L, ct3, keys, out=None):
        plan = self.plan
        batch = ct3.numel() // (3 * L * plan.n)
        if out is None:
            out = torch.empty((batch, 2, L, plan.n), dtype=torch.int64, device=ct3.device)
        ws = plan.workspace(plan.lib.troyn_relinearize_workspace_bytes(plan.h, L, batch))
        capi.check(plan.lib.troyn_bgv_relinearize(self.h, L, _ptr(ct3), plan._key_ptrs(keys, L), _ptr(out), C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    # -- hoisted rotations (additions: the Plan methods of the same names on NTT-form operands, with the BGV division as their tail;
    #    self must be the key level; the workspaces are the plan's queries with is_ntt_form = 1) --
    def apply_galois_many(self, L, ct, elements, keys_per_element, out=None):
        """ct [batch][2][L][N] -> [terms][batch][2][L][N], ONE digit decomposition of ct (include/troyn.h states the contract)"""
        return self.plan._apply_galois_hoisted(False, L, ct, elements, keys_per_element, False, True, out, bgv=self)

    def apply_galois_sum(self, L, ct, elements, keys_per_element, out=None):
        """ct [batch][2][L][N] -> [batch][2][L][N]: the sum over the elements, one decomposition and ONE division by the special prime"""
        return self.plan._apply_galois_hoisted(True, L, ct, elements, keys_per_element, False, True, out, bgv=self)

    def apply_galois_weighted_sums(self, L, ct, elements, keys_per_element, weights, out=None):
        """ct [batch][2][L][N] -> [slots][batch][2][L][N]: out[s] = SUM_t weights[s][t] (.) sigma_elements[t](ct), one division per slot;
        weights[s][t]: [K][N] NTT form, key-level layout, or None"""
        return self.plan._apply_galois_weighted_sums(L, ct, elements, keys_per_element, weights, False, True, out, bgv=self)

    def apply_galois_sum_each(self, L, cts, elements, keys_per_element, out=None):
        """cts [terms][batch][2][L][N] -> [batch][2][L][N]: SUM_t sigma_elements[t](cts[t]) with ONE division by the special prime"""
        return self.plan._apply_galois_sum_each(L, cts, elements, keys_per_element, False, True, out, bgv=self)

    def linear_transform_bsgs(self, L, ct, baby_elements, baby_keys, giant_elements, giant_keys, weights, out=None):
        """ct [batch][2][L][N] -> [batch][2][L][N]: SUM_g sigma_G[g]( SUM_b weights[g][b] (.) sigma_B[b](ct) ); word for word
        apply_galois_weighted_sums followed by apply_galois_sum_each"""
        return self.plan._linear_transform_bsgs("troyn_linear_transform_bsgs", L, ct, baby_elements, baby_keys, giant_elements, giant_keys,
                                                weights, False, True, out, bgv=self)

    def multiply_relinearize_mod_switch(self, level_handle, a, b, keys, out=None):
        """self must be the key level (L = plan.K), level_handle the Bgv of the operands' level L; a, b [batch][2][L][N] NTT form ->
        [batch][2][L-1][N], word for word dyadic_convolute + relinearize + level_handle.mod_t_and_divide_q_last_ntt.  The caller multiplies
        the product's correction factor by level_handle.inv_q_last_mod_t."""
        plan, L = self.plan, level_handle.L
        batch = a.numel() // (2 * L * plan.n)
        if out is None:
            out = torch.empty((batch, 2, L - 1, plan.n), dtype=torch.int64, device=a.device)
        ws = plan.workspace(plan.lib.troyn_bgv_multiply_relinearize_mod_switch_workspace_bytes(self.h, L, batch))
        capi.check(plan.lib.troyn_bgv_multiply_relinearize_mod_switch(self.h, level_handle.h, _ptr(a), _ptr(b), plan._key_ptrs(keys, L), _ptr(out),
                                                                      C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out


class Ring2k:
    """troyn_ring2k: PolynomialEncoderRNSHelper<T> (src/app/bfv_ring2k.cu) of the level with the plan's first L primes; elements are
    numpy arrays of uint32 / uint64, or uint64 pairs (low, high) for 128-bit elements."""

    def __init__(self, plan, L, t_bits, elem_bits):
        self.plan, self.L, self.t_bits, self.elem_bytes = plan, int(L), int(t_bits), elem_bits // 8
        h = C.c_void_p()
        capi.check(plan.lib.troyn_ring2k_create(C.byref(h), plan.h, self.L, self.t_bits, self.elem_bytes))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.plan.lib.troyn_ring2k_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def gamma(self):
        return int(self.plan.lib.troyn_ring2k_gamma(self.h))

    def _elements(self, values):
        """list of Python ints -> device byte buffer"""
        raw = b"".join(int(v).to_bytes(self.elem_bytes, "little") for v in values) or b"\0" * 16
        host = np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype=np.int64).copy()
        return torch.from_numpy(host).to(self.plan.device)

    def _encode(self, fn, values):
        buf = self._elements(values)
        out = torch.empty((self.L, self.plan.n), dtype=torch.int64, device=self.plan.device)
        capi.check(fn(self.h, _ptr(buf), len(values), _ptr(out), _stream()))
        return out

    def scale_up(self, values):
        return self._encode(self.plan.lib.troyn_ring2k_scale_up, values)

    def centralize(self, values):
        return self._encode(self.plan.lib.troyn_ring2k_centralize, values)

    def scale_down(self, phase):
        """phase [L][N] coefficient form -> list of N Python ints"""
        words = (self.plan.n * self.elem_bytes + 7) // 8
        out = torch.empty(words, dtype=torch.int64, device=self.plan.device)
        capi.check(self.plan.lib.troyn_ring2k_scale_down(self.h, _ptr(phase), _ptr(out), _stream()))
        raw = out.cpu().numpy().tobytes()
        return [int.from_bytes(raw[i * self.elem_bytes:(i + 1) * self.elem_bytes], "little") for i in range(self.plan.n)]

    def decentralize(self, plain, correction_factor=1):
        """plain [L][N] coefficient form (x mod Q) -> list of N Python ints x * correction_factor^-1 mod 2^k (bfv_ring2k.cu:872-925)"""
        words = (self.plan.n * self.elem_bytes + 7) // 8
        out = torch.empty(words, dtype=torch.int64, device=self.plan.device)
        cf = int(correction_factor)
        capi.check(self.plan.lib.troyn_ring2k_decentralize(self.h, _ptr(plain), _ptr(out), cf & ((1 << 64) - 1), (cf >> 64) & ((1 << 64) - 1), _stream()))
        raw = out.cpu().numpy().tobytes()
        return [int.from_bytes(raw[i * self.elem_bytes:(i + 1) * self.elem_bytes], "little") for i in range(self.plan.n)]


class CkksEncoder:
    """troyn_ckks: the CKKS encoder on the device (src/ckks_encoder.cu).  Values are torch.float64 CUDA tensors (complex values as [..][2] = re, im),
    plaintexts int64 tensors [batch][L][N] in NTT form under the plan's first L moduli."""

    def __init__(self, plan):
        self._plan = weakref.ref(plan)       # the plan may own this object (Plan.ckks_handle): no cycle between two objects with __del__
        self.lib = plan.lib
        h = C.c_void_p()
        capi.check(plan.lib.troyn_ckks_create(C.byref(h), plan.h))
        self.h = h

    @property
    def plan(self):
        plan = self._plan()
        if plan is None or not plan.h:
            raise capi.TroynError("[troyn] the plan of this CkksEncoder is gone")
        return plan

    def close(self):
        if getattr(self, "h", None):
            self.lib.troyn_ckks_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tables(self):
        """host copies: index_map uint32 [N], root_powers and inv_root_powers float64 [N][2]"""
        n = self.plan.n
        index_map, roots, inv_roots = np.zeros(n, dtype=np.uint32), np.zeros((n, 2), dtype=np.float64), np.zeros((n, 2), dtype=np.float64)
        capi.check(self.plan.lib.troyn_ckks_get_tables(self.h, C.c_void_p(index_map.ctypes.data), C.c_void_p(roots.ctypes.data), C.c_void_p(inv_roots.ctypes.data)))
        return index_map, roots, inv_roots

    def _f64(self, t):
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
            raise capi.TroynInvalidArgument("[troyn] values must be contiguous float64 CUDA tensors")
        return C.c_void_p(t.data_ptr())

    def _ws(self, nbytes):
        ws = self.plan.workspace(nbytes)
        return C.c_void_p(ws.data_ptr()), ws.numel()

    def _encode(self, fn, L, values, batch, count, scale, flags):
        out = torch.empty((batch, L, self.plan.n), dtype=torch.int64, device=self.plan.device)
        too_large = torch.empty(max(batch, 1), dtype=torch.int32, device=self.plan.device) if flags else None
        ws, ws_bytes = self._ws(self.lib.troyn_ckks_encode_workspace_bytes(self.h, batch))
        capi.check(fn(self.h, L, self._f64(values), count, float(scale), _ptr(out), C.c_void_p(too_large.data_ptr()) if flags else None, ws, ws_bytes, batch, _stream()))
        return (out, too_large[:batch]) if flags else out

    def encode_simd(self, L, values, scale, flags=False):
        """values [batch][count][2] -> [batch][L][N] (and the too_large flags, int32 [batch], with flags=True)"""
        batch, count = values.shape[0], values.shape[1]
        return self._encode(self.plan.lib.troyn_ckks_encode_simd, L, values, batch, count, scale, flags)

    def encode_diagonals(self, L, src, pairs, scale, n, matrix=False, flags=False):
        """troyn_ckks_encode_diagonals: src float64 [nd][n][2] (diagonals) or [n][n][2] (row-major matrix, matrix=True), pairs int32 [items][2] =
        (diagonal, shift) -> [items][L][N]: item t encodes the diagonal rotated back by its shift, repeated across the N/2 slots"""
        if pairs.dtype != torch.int32 or not pairs.is_contiguous() or not pairs.is_cuda or pairs.dim() != 2 or pairs.shape[1] != 2:
            raise capi.TroynInvalidArgument("[troyn] pairs must be a contiguous int32 CUDA tensor [items][2]")
        n = int(n)
        if src.dim() != 3 or src.shape[1] != n or src.shape[2] != 2 or (matrix and src.shape[0] != n):
            raise capi.TroynInvalidArgument("[troyn] src must be [nd][n][2] (diagonals) or [n][n][2] (matrix)")
        items, nd = pairs.shape[0], src.shape[0]
        out = torch.empty((items, L, self.plan.n), dtype=torch.int64, device=self.plan.device)
        too_large = torch.empty(max(items, 1), dtype=torch.int32, device=self.plan.device) if flags else None
        ws, ws_bytes = self._ws(self.lib.troyn_ckks_encode_diagonals_workspace_bytes(self.h, items))
        capi.check(self.lib.troyn_ckks_encode_diagonals(self.h, L, self._f64(src), 1 if matrix else 0, n, nd, C.c_void_p(pairs.data_ptr()), float(scale), _ptr(out),
                                                        C.c_void_p(too_large.data_ptr()) if flags else None, ws, ws_bytes, items, _stream()))
        return (out, too_large[:items]) if flags else out

    def dft_factor_diagonals(self, first, count, inverse=False, col_mask=0, row_mask=0, conjugate=False, constant=1.0):
        """troyn_ckks_dft_factor_diagonals: the product of the layers [first, first + count) of the special DFT (CoeffToSlot / SlotToCoeff) by its
        present diagonals -> float64 [nd][N/2][2], the source of encode_diagonals; masks: 0 none, 1 even, 2 odd"""
        nd = int(self.lib.troyn_ckks_dft_factor_diagonals_count(self.h, first, count))
        out = torch.empty((nd, self.plan.n // 2, 2), dtype=torch.float64, device=self.plan.device)
        capi.check(self.lib.troyn_ckks_dft_factor_diagonals(self.h, first, count, 1 if inverse else 0, int(col_mask), int(row_mask), 1 if conjugate else 0,
                                                            float(constant), C.c_void_p(out.data_ptr()), _stream()))
        return out

    def dft_factor_diagonals_sparse(self, n, first, count, inverse=False, col_mask=0, row_mask=0, conjugate=False, constant=1.0):
        """troyn_ckks_dft_factor_diagonals_sparse: the same product on the sub-ring of n <= N/2 slots (sparse packing), log2 n layers in all
        -> float64 [nd][n][2], the source of encode_diagonals with that n"""
        n = int(n)
        nd = int(self.lib.troyn_ckks_dft_factor_diagonals_sparse_count(self.h, n, first, count))
        out = torch.empty((nd, n if nd else 0, 2), dtype=torch.float64, device=self.plan.device)
        capi.check(self.lib.troyn_ckks_dft_factor_diagonals_sparse(self.h, n, first, count, 1 if inverse else 0, int(col_mask), int(row_mask), 1 if conjugate else 0,
                                                                   float(constant), C.c_void_p(out.data_ptr()), _stream()))
        return out

    def dft_factor_diagonals_packed(self, n, first, count, inverse=False, constant=1.0):
        """troyn_ckks_dft_factor_diagonals_packed: layers [first, first + count) of the n-slot transform on 2n rows (n <= N/4), rows >= n turned by -i
        (inverse) / +i (forward) -> float64 [nd][2n][2], the source of encode_diagonals with n = 2n"""
        n = int(n)
        nd = int(self.lib.troyn_ckks_dft_factor_diagonals_packed_count(self.h, n, first, count))
        out = torch.empty((nd, 2 * n if nd else 0, 2), dtype=torch.float64, device=self.plan.device)
        capi.check(self.lib.troyn_ckks_dft_factor_diagonals_packed(self.h, n, first, count, 1 if inverse else 0, float(constant), C.c_void_p(out.data_ptr()), _stream()))
        return out

    def encode_polynomial(self, L, coeffs, scale, flags=False):
        """coeffs [batch][count] -> [batch][L][N]"""
        batch, count = coeffs.shape[0], coeffs.shape[1]
        return self._encode(self.plan.lib.troyn_ckks_encode_polynomial, L, coeffs, batch, count, scale, flags)

    def _decode(self, fn, L, plain, scale, shape):
        batch = plain.numel() // (L * self.plan.n)
        out = torch.empty((batch,) + shape, dtype=torch.float64, device=self.plan.device)
        ws, ws_bytes = self._ws(self.lib.troyn_ckks_workspace_bytes(self.h, L, batch))
        capi.check(fn(self.h, L, _ptr(plain), float(scale), C.c_void_p(out.data_ptr()), ws, ws_bytes, batch, _stream()))
        return out

    def decode_polynomial(self, L, plain, scale):
        """plain [batch][L][N] NTT form -> float64 [batch][N]"""
        return self._decode(self.plan.lib.troyn_ckks_decode_polynomial, L, plain, scale, (self.plan.n,))

    def decode_simd(self, L, plain, scale):
        """plain [batch][L][N] NTT form -> float64 [batch][N/2][2]"""
        return self._decode(self.plan.lib.troyn_ckks_decode_simd, L, plain, scale, (self.plan.n // 2, 2))

    def mod_raise(self, rows, L_in, L_out, pcount, is_ntt_form):
        """troyn_ckks_mod_raise: rows int64 [batch][pcount][L_in][N] -> [batch][pcount][L_out][N], the residues of the centred representative of
        every coefficient modulo the plan's first L_out moduli (rows below L_in unchanged)"""
        n = self.plan.n
        batch = rows.numel() // (pcount * L_in * n)
        out = torch.empty((batch, pcount, L_out, n), dtype=torch.int64, device=self.plan.device)
        ws, ws_bytes = self._ws(self.lib.troyn_ckks_mod_raise_workspace_bytes(self.h, L_in, L_out, pcount, batch, 1 if is_ntt_form else 0))
        capi.check(self.lib.troyn_ckks_mod_raise(self.h, L_in, L_out, 1 if is_ntt_form else 0, _ptr(rows), pcount, _ptr(out), ws, ws_bytes, batch, _stream()))
        return out


class Behz:
    """troyn_behz: BEHZ constants (RNSTool, utils/rns_tool.cu:29-275) for level L and plain modulus t."""

    def __init__(self, plan, L, plain_modulus):
        self.plan, self.L, self.t = plan, int(L), int(plain_modulus)
        h = C.c_void_p()
        capi.check(plan.lib.troyn_behz_create(C.byref(h), plan.h, self.L, self.t))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.plan.lib.troyn_behz_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def base_Bsk(self):
        n = self.plan.lib.troyn_behz_base_Bsk_size(self.h)
        out = np.zeros(n, dtype=np.uint64)
        capi.check(self.plan.lib.troyn_behz_get_base_Bsk(self.h, out.ctypes.data_as(capi.p64)))
        return [int(x) for x in out]

    @property
    def working_base_size(self):
        """primes of the auxiliary base the multiply works in (more, smaller primes than base_Bsk when every q_i is below 2^50)"""
        return int(self.plan.lib.troyn_behz_working_base_size(self.h))

    @property
    def gamma(self):
        return int(self.plan.lib.troyn_behz_gamma(self.h))

    def scale_up(self, plain, src=None, subtract=False, out=None):
        """plain [batch][N] mod t -> out [batch][L][N] = (src or 0) +/- round(q/t * plain)   (scaling_variant::scale_up)"""
        n, L = self.plan.n, self.L
        batch = plain.numel() // n
        if out is None:
            out = torch.empty((batch, L, n), dtype=torch.int64, device=plain.device)
        capi.check(self.plan.lib.troyn_bfv_scale_up(self.h, _ptr(plain), n, n, _ptr(src) if src is not None else None, L * n,
                                                    _ptr(out), L * n, int(subtract), batch, _stream()))
        return out

    def decrypt_scale_and_round(self, phase, out=None):
        """phase [batch][L][N] -> [batch][N] mod t   (RNSTool::decrypt_scale_and_round)"""
        n, L = self.plan.n, self.L
        batch = phase.numel() // (L * n)
        if out is None:
            out = torch.empty((batch, n), dtype=torch.int64, device=phase.device)
        capi.check(self.plan.lib.troyn_bfv_decrypt_scale_and_round(self.h, _ptr(phase), _ptr(out), batch, _stream()))
        return out

    def multiply(self, a, pa, b, pb, out=None):
        """a [batch][pa][L][N] x b [batch][pb][L][N] (coefficient form) -> [batch][pa+pb-1][L][N]"""
        n, L = self.plan.n, self.L
        batch = a.numel() // (pa * L * n)
        if out is None:
            out = torch.empty((batch, pa + pb - 1, L, n), dtype=torch.int64, device=a.device)
        nbytes = self.plan.lib.troyn_bfv_multiply_workspace_bytes(self.h, pa, pb, batch)
        ws = self.plan.workspace(nbytes)
        capi.check(self.plan.lib.troyn_bfv_multiply(self.h, _ptr(a), pa, _ptr(b), pb, _ptr(out),
                                                    C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out

    # -- inner product: a sum of tensor products, one scale-down (additions) ------------------------------
    def bfv_multiply_accumulate(self, a_list, b_list, out=None):
        """SUM_t a_list[t] x b_list[t] -> [batch][3][L][N]; operands [batch][2][L][N] in coefficient form; one floor for the sum"""
        n, L = self.plan.n, self.L
        pa, pb, batch = self.plan._term_ptrs("[troyn_bfv_multiply_accumulate]", a_list, b_list, 2 * L * n)
        if out is None:
            out = torch.empty((batch, 3, L, n), dtype=torch.int64, device=self.plan.device)
        nbytes = self.plan.lib.troyn_bfv_multiply_accumulate_workspace_bytes(self.h, len(a_list), batch)
        ws = self.plan.workspace(nbytes)
        capi.check(self.plan.lib.troyn_bfv_multiply_accumulate(self.h, pa, pb, len(a_list), _ptr(out), C.c_void_p(ws.data_ptr()), ws.numel(),
                                                               batch, _stream()))
        return out

    def bfv_multiply_accumulate_relinearize(self, a_list, b_list, keys, out=None):
        """relinearize(SUM_t a_list[t] x b_list[t]) -> [batch][2][L][N]: one floor and one key switch for the sum"""
        n, L = self.plan.n, self.L
        pa, pb, batch = self.plan._term_ptrs("[troyn_bfv_multiply_accumulate_relinearize]", a_list, b_list, 2 * L * n)
        if out is None:
            out = torch.empty((batch, 2, L, n), dtype=torch.int64, device=self.plan.device)
        nbytes = self.plan.lib.troyn_bfv_multiply_accumulate_relinearize_workspace_bytes(self.h, len(a_list), batch)
        ws = self.plan.workspace(nbytes)
        capi.check(self.plan.lib.troyn_bfv_multiply_accumulate_relinearize(self.h, pa, pb, len(a_list), self.plan._key_ptrs(keys, L), _ptr(out),
                                                                           C.c_void_p(ws.data_ptr()), ws.numel(), batch, _stream()))
        return out
