"""Device-resident scoring: spectra stay in HBM, results land in HBM, caller owns the stream.

Thin Python front for the pya_plan_* entry points of include/pyascore_hip.h.  PyTorch is used
only as plumbing (device allocations, the current HIP stream, torch.distributed); nothing here
computes with torch.
"""
import ctypes as C

import numpy as np

from . import _lib
from .ascore import PyAscore, _as_ptr
from .ranked import check_k as check_ranked_k


class DevicePlan:
    """One batch planned once (host pre-pass, tables, workspace), runnable many times.

    ``spectra`` are two float64 or float32 CUDA/HIP tensors (m/z, intensity) laid out as the batch's
    ``peak_off`` says (a batch with ``spec_of``: the spectra's, each held once and shared by its PSMs,
    which must be consecutive).  ``run()`` enqueues the three kernels on torch's current stream and
    returns the result tensors (device).  ``max_k`` widens the per-site result rows beyond this
    batch's own largest n_of_mod: ranks that gather fixed-size records pass the job-wide value.
    ``evidence()`` after ``run()`` gives the evidence records of every site (``pya_plan_evidence``); ``evidence=True``
    tells the plan at creation that they will be asked for (a plan of a handful of PSMs then takes the per-stage
    launches instead of the one-launch kernel).  ``ions()`` / ``ions=True``: the same for the ion records
    (``pya_plan_ions_count``, ``pya_plan_ions``).  ``named()`` / ``named=True``: the same for the records of localisations
    the caller names (``pya_plan_named``).  ``sites()`` / ``sites=True``: the same for the site tables
    (``pya_plan_site_offsets``, ``pya_plan_sites``).  ``probs()`` / ``probs=True``: the same for the site probabilities
    (``pya_plan_probs``).  ``ranked()`` / ``ranked=True``: the same for the ranked localisations (``pya_plan_ranked``).  ``rollup()`` /
    ``rollup=True``: the probability records rolled into a table of the caller's slots (``pya_plan_rollup``).
    ``peptidoforms()`` / ``peptidoforms=True``: the PSMs collapsed onto one record per (group, best_sig)
    (``pya_plan_peptidoforms``); ``peptidoform_reduce()`` merges such lists.  ``mz_profile()`` / ``mz_profile=True``: the
    fragment mass errors of the reported localisations binned per run slot (``pya_plan_mz_profile``).  ``coverage()`` /
    ``coverage=True``: per PSM the ion current of its spectrum and the part the reported localisation explains (``pya_plan_coverage``).
    ``site_quant()`` / ``quant=True``: the channel intensities of a device matrix summed per roll-up slot over the confidently
    localised records (``pya_plan_site_quant``; ``pyascore_amd.device.marker_values`` makes the matrix from marker records).
    ``fit_mz_calibration()`` turns such a table into an m/z calibration and ``recalibrate()`` corrects a device m/z tensor with
    it (``pya_mz_profile_fit``, ``pya_recalibrate_spectra``), so run -> profile -> fit -> correct -> run again needs no host copy.

    A plan belongs to the settings it was made under: after ``scorer.add_neutral_loss`` its ``run()`` and every stage method
    raise ``RuntimeError`` ("settings changed since the plan was made") with nothing enqueued -- make a new plan.  ``check()``,
    ``site_offsets()``, the timings and the result tensors of the runs so far stay valid."""

    def __init__(self, scorer, batch, timing=False, max_k=None, evidence=False, ions=False, named=False, sites=False, probs=False,
                 ranked=False, rollup=False, peptidoforms=False, mz_profile=False, coverage=False, quant=False, peptidoform_quant=False):
        import torch
        if not isinstance(scorer, PyAscore):
            raise TypeError("scorer must be a pyascore_amd.PyAscore")
        self._torch = torch
        self.scorer = scorer
        self._lib = scorer._lib
        self.n_psm = int(batch["n_psm"])
        self.max_k = max(1, int(np.max(batch["n_of_mod"]))) if self.n_psm else 1
        if max_k is not None:
            if int(max_k) < self.max_k:
                raise ValueError("max_k=%d is smaller than the batch's largest n_of_mod (%d)" % (max_k, self.max_k))
            self.max_k = int(max_k)
        self.device = torch.device("cuda", scorer.device)
        self._meta = dict(
            peak_off=np.ascontiguousarray(batch["peak_off"], np.int64),
            pep=np.ascontiguousarray(batch["pep"], np.uint8),
            pep_off=np.ascontiguousarray(batch["pep_off"], np.int64),
            n_of_mod=np.ascontiguousarray(batch["n_of_mod"], np.int32),
            max_charge=np.ascontiguousarray(batch["max_charge"], np.int32),
            aux_pos=np.ascontiguousarray(batch["aux_pos"], np.uint32),
            aux_mass=np.ascontiguousarray(batch["aux_mass"], np.float32),
            aux_off=np.ascontiguousarray(batch["aux_off"], np.int64))
        m = self._meta
        b = _lib.Batch(self.n_psm, _as_ptr(m["peak_off"]), _as_ptr(m["pep"]), _as_ptr(m["pep_off"]),
                       _as_ptr(m["n_of_mod"]), _as_ptr(m["max_charge"]), _as_ptr(m["aux_pos"]),
                       _as_ptr(m["aux_mass"]), _as_ptr(m["aux_off"]))
        self._plan = C.c_void_p()
        flags = (_lib.PYA_FLAG_TIMING if timing else 0) | (_lib.PYA_FLAG_EVIDENCE if evidence else 0) | \
            (_lib.PYA_FLAG_IONS if ions else 0) | (_lib.PYA_FLAG_NAMED if named else 0) | (_lib.PYA_FLAG_SITES if sites else 0) | \
            (_lib.PYA_FLAG_PROBS if probs else 0) | (_lib.PYA_FLAG_RANKED if ranked else 0) | \
            (_lib.PYA_FLAG_ROLLUP if rollup else 0) | (_lib.PYA_FLAG_PEPTIDOFORMS if peptidoforms else 0) | \
            (_lib.PYA_FLAG_MZ_PROFILE if mz_profile else 0) | (_lib.PYA_FLAG_COVERAGE if coverage else 0) | \
            (_lib.PYA_FLAG_QUANT if quant else 0) | (_lib.PYA_FLAG_PFORM_QUANT if peptidoform_quant else 0)
        if batch.get("spec_of") is not None:
            # shared spectra (synth.pack_shared_batch): peak_off describes the spectra, spec_of names every PSM's
            spec_of = m["spec_of"] = np.ascontiguousarray(batch["spec_of"], np.uint32)
            n_spec = int(batch.get("n_spectra", m["peak_off"].size - 1))
            if spec_of.size != self.n_psm or m["peak_off"].size != n_spec + 1:
                raise ValueError("a shared batch has one spec_of entry per PSM and n_spectra + 1 peak offsets")
            rc = self._lib.pya_plan_create_shared(scorer._h, C.byref(b), _as_ptr(spec_of), n_spec, flags, C.byref(self._plan))
        else:
            rc = self._lib.pya_plan_create(scorer._h, C.byref(b), flags, C.byref(self._plan))
        if rc:
            self._plan = None
            scorer._raise(rc)
        self.timing = timing
        n, k = self.n_psm, self.max_k
        with torch.cuda.device(self.device):
            self.best_score = torch.empty(n, dtype=torch.float32, device=self.device)
            self.best_sig = torch.empty(n, dtype=torch.int64, device=self.device)     # u64 bit patterns
            self.n_sig = torch.empty(n, dtype=torch.int32, device=self.device)
            self.ascores = torch.empty((n, k), dtype=torch.float32, device=self.device)
            self.alt_mask = torch.empty((n, k), dtype=torch.int64, device=self.device)
        self._res = _lib.Results(k, self.best_score.data_ptr(), self.best_sig.data_ptr(), self.n_sig.data_ptr(),
                                 self.ascores.data_ptr(), self.alt_mask.data_ptr())

    def close(self):
        if getattr(self, "_plan", None) is not None and self._plan.value:
            self._lib.pya_plan_destroy(self._plan)
            self._plan = C.c_void_p()

    __del__ = close

    @property
    def workspace_bytes(self):
        return int(self._lib.pya_plan_workspace_bytes(self._plan))

    @property
    def total_signatures(self):
        return int(self._lib.pya_plan_total_signatures(self._plan))

    def run(self, d_mz, d_intensity):
        """Enqueues the plan on torch's current stream.  The tensors are float64, or typed: float64 m/z with float32
        intensities, or both float32 (the binning kernels widen at the load; results as for the widened tensors, bit for
        bit).  One plan takes any of the three from run to run."""
        torch = self._torch
        for t in (d_mz, d_intensity):
            if t.dtype not in (torch.float64, torch.float32) or not t.is_cuda or not t.is_contiguous():
                raise ValueError("spectra must be contiguous float64 device tensors (or float32: float64 m/z with float32 "
                                 "intensities, or both float32)")
        if d_mz.dtype == torch.float32 and d_intensity.dtype == torch.float64:
            raise ValueError("spectra must be contiguous float64 device tensors (float32 m/z beside float64 intensities is "
                             "not supported)")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if d_intensity.dtype == torch.float64:
            rc = self._lib.pya_plan_run(self._plan, d_mz.data_ptr(), d_intensity.data_ptr(), stream, C.byref(self._res))
        else:
            sp = _lib.TypedSpectra(d_mz.data_ptr(), d_intensity.data_ptr(), _lib.spectrum_type(d_mz.dtype),
                                   _lib.spectrum_type(d_intensity.dtype))
            rc = self._lib.pya_plan_run_typed(self._plan, C.byref(sp), stream, C.byref(self._res))
        if rc:
            self.scorer._raise(rc)
        return self

    def evidence(self, out=None):
        """The evidence records of the last ``run()`` as a ``torch.uint8`` device tensor ``[n_psm, max_k, 16]`` (one
        16-byte ``pya_evidence`` per modified site, rows as ``ascores``): ONE launch family of the library behind the run,
        on torch's current stream.  Valid for the results of the last run; ``evidence_rows`` turns a host copy into the
        structured array."""
        torch = self._torch
        shape = (self.n_psm, self.max_k, 16)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous uint8 device tensor of shape %r" % (shape,))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.pya_plan_evidence(self._plan, C.byref(self._res), stream, out.data_ptr())
        if rc:
            self.scorer._raise(rc)
        return out

    def ions(self, cap=None):
        """The ion records of the last ``run()``: ``(ion_off, records)``, an ``int64`` device tensor ``[n_psm + 1]`` and a
        ``torch.uint8`` device tensor ``[total, 16]`` (one 16-byte ``pya_ion`` each; ``ion_records`` turns a host copy into
        the structured array).  Count and scan are enqueued on torch's current stream; the one wait is this method reading
        the total to allocate (a caller that knows a bound passes ``cap`` and nothing waits: ``records`` then has ``cap``
        rows, ``check()`` reports a PSM that did not fit).  Valid for the results of the last run."""
        torch = self._torch
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            off = torch.empty(self.n_psm + 1, dtype=torch.int64, device=self.device)
            rc = self._lib.pya_plan_ions_count(self._plan, C.byref(self._res), stream, off.data_ptr())
            if rc:
                self.scorer._raise(rc)
            total = int(off[-1].item()) if cap is None else int(cap)
            out = torch.zeros((total, 16), dtype=torch.uint8, device=self.device)
        if total and self.n_psm:
            rc = self._lib.pya_plan_ions(self._plan, C.byref(self._res), stream, off.data_ptr(), out.data_ptr(), total)
            if rc:
                self.scorer._raise(rc)
        return off, out

    def named(self, q_off, sig_bits, counts=False, scores=False):
        """The named-localisation records of the last ``run()`` for the queries ``q_off`` (int64 device tensor
        ``[n_psm + 1]``) / ``sig_bits`` (int64 device tensor holding the uint64 bit patterns, ``[n_q]``): a ``torch.uint8``
        device tensor ``[n_q, 32]`` (one ``pya_named`` each; ``named_records`` turns a host copy into the structured array),
        or ``(records, counts, scores)`` with ``counts`` int32 / ``scores`` float32 ``[n_q, n_top]`` (``None`` where not
        asked for).  One launch family of the library behind the run on torch's current stream; nothing waits on the host:
        the size of the output is ``sig_bits.numel()``, and no write passes it whatever ``q_off`` holds (``check()``
        reports a PSM whose range does).  Valid for the results of the last run; may be called again with other queries."""
        torch = self._torch
        for t, what in ((q_off, "q_off"), (sig_bits, "sig_bits")):
            if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
                raise ValueError("%s must be a contiguous one-dimensional int64 device tensor" % what)
        if q_off.numel() != self.n_psm + 1:
            raise ValueError("q_off must have n_psm + 1 entries")
        n_q, n_top = int(sig_bits.numel()), self.scorer._n_top
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            out = torch.zeros((n_q, 32), dtype=torch.uint8, device=self.device)
            d_counts = torch.zeros((n_q, n_top), dtype=torch.int32, device=self.device) if counts else None
            d_scores = torch.zeros((n_q, n_top), dtype=torch.float32, device=self.device) if scores else None
        rc = self._lib.pya_plan_named(self._plan, C.byref(self._res), stream, q_off.data_ptr(), sig_bits.data_ptr(), n_q,
                                      out.data_ptr(), d_counts.data_ptr() if counts else None,
                                      d_scores.data_ptr() if scores else None)
        if rc:
            self.scorer._raise(rc)
        return (out, d_counts, d_scores) if counts or scores else out

    def site_offsets(self):
        """``site_off`` (int64 numpy ``[n_psm + 1]``): where the site records of every PSM lie.  Known from the plan's host
        pre-pass, so it needs no run and nothing on the device."""
        off = np.zeros(self.n_psm + 1, np.int64)
        rc = self._lib.pya_plan_site_offsets(self._plan, _as_ptr(off))
        if rc:
            self.scorer._raise(rc)
        return off

    def sites(self, sig_cap=0, out=None):
        """The site table of the last ``run()``: ``(site_off, records)``, the host offsets of ``site_offsets()`` and a
        ``torch.uint8`` device tensor ``[site_off[-1], 32]`` (one ``pya_site`` per modifiable residue; ``site_records``
        turns a host copy into the structured array).  One launch family of the library behind the run on torch's current
        stream; nothing waits on the host.  ``sig_cap``: PSMs with more site assignments get ``PYA_SITE_OVER`` records
        (0: no cap).  Valid for the results of the last run; may be called again."""
        torch = self._torch
        off = self.site_offsets()
        shape = (int(off[-1]), 32)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.zeros(shape, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous uint8 device tensor of shape %r" % (shape,))
        rc = self._lib.pya_plan_sites(self._plan, C.byref(self._res), stream, int(sig_cap), out.data_ptr())
        if rc:
            self.scorer._raise(rc)
        return off, out

    def probs(self, sig_cap=0, out=None):
        """The site probabilities of the last ``run()``: ``(site_off, site_probs, psm_probs)`` -- the host offsets of
        ``site_offsets()``, a ``torch.float64`` device tensor ``[site_off[-1], 2]`` (``with_prob``, ``without_prob`` per
        modifiable residue) and a ``torch.uint8`` device tensor ``[n_psm, 16]`` (one ``pya_psm_prob`` each; ``psm_prob_records``
        turns a host copy into the structured array).  One launch family of the library behind the run on torch's current
        stream; nothing waits on the host.  ``sig_cap`` as for ``sites()``; ``out``: the two tensors of an earlier call, to be
        written again.  Valid for the results of the last run."""
        torch = self._torch
        off = self.site_offsets()
        shapes = ((int(off[-1]), 2), (self.n_psm, 16))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if out is None:
            with torch.cuda.device(self.device):
                out = (torch.zeros(shapes[0], dtype=torch.float64, device=self.device),
                       torch.zeros(shapes[1], dtype=torch.uint8, device=self.device))
        site_probs, psm_probs = out
        for t, shape, dtype in ((site_probs, shapes[0], torch.float64), (psm_probs, shapes[1], torch.uint8)):
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("out must be contiguous device tensors: float64 %r and uint8 %r" % shapes)
        rc = self._lib.pya_plan_probs(self._plan, C.byref(self._res), stream, int(sig_cap), site_probs.data_ptr(), psm_probs.data_ptr())
        if rc:
            self.scorer._raise(rc)
        return off, site_probs, psm_probs

    def ranked(self, top_k=5, sig_cap=0, out=None):
        """The ranked localisations of the last ``run()``: a ``torch.uint8`` device tensor ``[n_psm, top_k, 16]`` (one
        ``pya_ranked`` per row; ``ranked_records`` turns a host copy into the structured array ``[n_psm, top_k]``) -- row 0 of
        a PSM its reported localisation, then its other site assignments by PepScore descending, equal scores by ascending
        sig bits.  One launch family of the library behind the run on torch's current stream; nothing waits on the host.
        ``top_k``: 1 .. 64; ``sig_cap`` as for ``sites()``; ``out``: the tensor of an earlier call with the same ``top_k``, to
        be written again.  Valid for the results of the last run; may be called again, with another ``top_k`` too."""
        torch = self._torch
        top_k = check_ranked_k(top_k)
        shape = (self.n_psm, top_k, 16)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.zeros(shape, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous uint8 device tensor of shape %r" % (shape,))
        rc = self._lib.pya_plan_ranked(self._plan, C.byref(self._res), stream, top_k, int(sig_cap), out.data_ptr())
        if rc:
            self.scorer._raise(rc)
        return out

    def rollup_clear(self, n_slots=None, table=None):
        """A roll-up table in the empty state: a ``torch.uint8`` device tensor ``[n_slots, 32]`` (one ``pya_site_rollup`` per
        slot; ``rollup_records`` turns a host copy into the structured array), new or -- ``table`` -- an earlier one to be
        emptied again.  One launch on torch's current stream.  The empty slot is not all-zero bytes (``best_psm`` is "no
        PSM"): a table must come from here before ``rollup()`` accumulates into it."""
        torch = self._torch
        if table is None:
            with torch.cuda.device(self.device):
                table = torch.empty((int(n_slots), 32), dtype=torch.uint8, device=self.device)
        if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != 32 or not table.is_contiguous() or not table.is_cuda:
            raise ValueError("table must be a contiguous uint8 device tensor of shape (n_slots, 32)")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.pya_rollup_clear(self.scorer._h, table.data_ptr(), table.shape[0], stream)
        if rc:
            self.scorer._raise(rc)
        return table

    def rollup(self, site_probs, psm_probs, slot, table, threshold=0.75, psm_id=None, psm_base=0):
        """Rolls the probability records of the last ``run()`` -- the two tensors of ``probs()`` -- into ``table`` (of
        ``rollup_clear``), which ACCUMULATES: the same table takes other plans, runs and calls, and the bytes are those of one
        call over all of their PSMs.  ``slot``: ``torch.int32`` device tensor, one entry per residue record
        (``site_offsets()[-1]``), the slot the record goes to, negative to leave it out; ``psm_id``: ``torch.int32`` /
        ``torch.uint32`` device tensor ``[n_psm]``, the numbers the PSMs are known by in ``best_psm``, or None: PSM i is
        ``psm_base + i``.  Two launches of the library on torch's current stream; nothing waits on the host.  A slot at or
        above the table's size writes nothing and is reported by ``check()``.  Returns ``table``."""
        torch = self._torch
        n_rec = int(self.site_offsets()[-1])
        if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != 32 or not table.is_contiguous() or not table.is_cuda:
            raise ValueError("table must be a contiguous uint8 device tensor of shape (n_slots, 32)")
        if slot.dtype != torch.int32 or tuple(slot.shape) != (n_rec,) or not slot.is_contiguous() or not slot.is_cuda:
            raise ValueError("slot must be a contiguous int32 device tensor of %d entries" % n_rec)
        if site_probs.dtype != torch.float64 or tuple(site_probs.shape) != (n_rec, 2) or not site_probs.is_contiguous() or not site_probs.is_cuda \
                or psm_probs.dtype != torch.uint8 or tuple(psm_probs.shape) != (self.n_psm, 16) or not psm_probs.is_contiguous() or not psm_probs.is_cuda:
            raise ValueError("site_probs and psm_probs must be the tensors of probs()")
        if psm_id is not None and (psm_id.element_size() != 4 or psm_id.is_floating_point() or tuple(psm_id.shape) != (self.n_psm,)
                                   or not psm_id.is_contiguous() or not psm_id.is_cuda):
            raise ValueError("psm_id must be a contiguous 32-bit integer device tensor of %d entries" % self.n_psm)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.pya_plan_rollup(self._plan, C.byref(self._res), stream, site_probs.data_ptr(), psm_probs.data_ptr(), slot.data_ptr(),
                                       table.shape[0], float(threshold), None if psm_id is None else psm_id.data_ptr(), int(psm_base),
                                       table.data_ptr())
        if rc:
            self.scorer._raise(rc)
        return table

    def site_quant(self, site_probs, psm_probs, slot, values, params, n_slots=None, row=None, row_base=0, table=None):
        """Adds the channel intensities of the contributing records of the last ``run()`` to ``table``
        (``pya_plan_site_quant``): a pair of ``torch.uint8`` device tensors ``[n_slots, 8]`` and ``[n_slots, n_channels, 16]``
        (one ``pya_site_quant_head`` per slot, one ``pya_site_quant`` per slot and channel; ``site_quant_records`` turns host
        copies into the structured arrays), new and zeroed when None -- ``n_slots`` of them.  The stage ACCUMULATES: the same
        table takes other plans, runs and calls, and an empty table is all-zero bytes.  ``site_probs`` / ``psm_probs``: the
        two tensors of ``probs()``; ``slot`` as for ``rollup()``; ``values``: contiguous ``torch.float64`` device tensor
        ``[n_rows, n_channels]``; ``params``: ``pyascore_amd.rollup.site_quant_params(...)``; ``row``: ``torch.int32`` device
        tensor ``[n_psm]``, the row of every PSM (negative: left out), or None: PSM i has row ``row_base + i``.  One launch on
        torch's current stream; nothing waits on the host.  A record that would contribute but names a slot or a row outside
        the table or the matrix writes nothing and is reported by ``check()``.  Returns ``table``."""
        from .rollup import site_quant_c_params
        torch = self._torch
        c_params = site_quant_c_params(params)
        n_ch = int(c_params.n_channels)
        n_rec = int(self.site_offsets()[-1])
        if table is None:
            if n_slots is None:
                raise ValueError("site_quant needs a table or n_slots")
            with torch.cuda.device(self.device):
                table = (torch.zeros((int(n_slots), 8), dtype=torch.uint8, device=self.device),
                         torch.zeros((int(n_slots), n_ch, 16), dtype=torch.uint8, device=self.device))
        head, cell = table
        if head.dtype != torch.uint8 or head.dim() != 2 or head.shape[1] != 8 or not head.is_contiguous() or not head.is_cuda \
                or cell.dtype != torch.uint8 or tuple(cell.shape) != (head.shape[0], n_ch, 16) or not cell.is_contiguous() or not cell.is_cuda:
            raise ValueError("table must be a pair of contiguous uint8 device tensors of shapes (n_slots, 8) and (n_slots, %d, 16)" % n_ch)
        if slot.dtype != torch.int32 or tuple(slot.shape) != (n_rec,) or not slot.is_contiguous() or not slot.is_cuda:
            raise ValueError("slot must be a contiguous int32 device tensor of %d entries" % n_rec)
        if site_probs.dtype != torch.float64 or tuple(site_probs.shape) != (n_rec, 2) or not site_probs.is_contiguous() or not site_probs.is_cuda \
                or psm_probs.dtype != torch.uint8 or tuple(psm_probs.shape) != (self.n_psm, 16) or not psm_probs.is_contiguous() or not psm_probs.is_cuda:
            raise ValueError("site_probs and psm_probs must be the tensors of probs()")
        if values.dtype != torch.float64 or values.dim() != 2 or values.shape[1] != n_ch or not values.is_contiguous() or not values.is_cuda:
            raise ValueError("values must be a contiguous float64 device tensor of shape (n_rows, %d)" % n_ch)
        if row is not None and (row.dtype != torch.int32 or tuple(row.shape) != (self.n_psm,) or not row.is_contiguous() or not row.is_cuda):
            raise ValueError("row must be a contiguous int32 device tensor of %d entries" % self.n_psm)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.pya_plan_site_quant(self._plan, C.byref(self._res), stream, site_probs.data_ptr(), psm_probs.data_ptr(), slot.data_ptr(),
                                           head.shape[0], values.data_ptr() if values.shape[0] else None, values.shape[0],
                                           None if row is None else row.data_ptr(), int(row_base), C.byref(c_params),
                                           head.data_ptr() if head.shape[0] else None, cell.data_ptr() if head.shape[0] else None)
        if rc:
            self.scorer._raise(rc)
        return table

    def rollup_flr(self, table, cls=None, reported_only=False):
        """Site FLR of the roll-up table (of ``rollup_clear()`` / ``rollup()``), where it lies (``pya_rollup_flr``): ``cls`` a
        ``torch.uint8`` device tensor of one byte per slot (0 target, 1 decoy, 2 left out) or None.  Returns device tensors
        ``(records, order, n_ranked)``: ``torch.uint8 [n_slots, 32]`` (one ``pya_site_flr`` per slot; ``flr_records`` turns a
        host copy into the structured array), the slots in order as ``torch.int32 [n_slots]`` (the bits of a uint32), and
        ``torch.int32 [2]``: the number of ranked slots and the number of class bytes that are none of 0, 1, 2.  The
        workspace is a torch tensor that lives for the call; everything is launched on torch's current stream and nothing
        waits on the host.  The table is only read."""
        torch = self._torch
        if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != 32 or not table.is_contiguous() or not table.is_cuda:
            raise ValueError("table must be a contiguous uint8 device tensor of shape (n_slots, 32)")
        n = int(table.shape[0])
        if cls is not None and (cls.dtype != torch.uint8 or tuple(cls.shape) != (n,) or not cls.is_contiguous() or not cls.is_cuda):
            raise ValueError("cls must be a contiguous uint8 device tensor of %d entries" % n)
        work_bytes = int(self._lib.pya_flr_workspace_bytes(n))
        with torch.cuda.device(self.device):
            work = torch.empty(max(work_bytes, 1), dtype=torch.uint8, device=self.device)
            records = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
            order = torch.empty(n, dtype=torch.int32, device=self.device)
            n_ranked = torch.empty(2, dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device)
        rc = self._lib.pya_rollup_flr(self.scorer._h, table.data_ptr(), n, None if cls is None else cls.data_ptr(),
                                      _lib.PYA_FLR_REPORTED_ONLY if reported_only else 0, stream.cuda_stream, work.data_ptr(), work_bytes,
                                      records.data_ptr(), order.data_ptr(), n_ranked.data_ptr())
        if rc:
            self.scorer._raise(rc)
        work.record_stream(stream)                 # (the caching allocator must not hand the workspace on before the stream is past it)
        return records, order, n_ranked

    def _pform_records(self, t, what):
        torch = self._torch
        if t is None:
            return None, 0
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != 48 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("%s must be a contiguous uint8 device tensor of shape (n, 48)" % what)
        return t, int(t.shape[0])

    def _pform_buffers(self, n_entries, cap):
        torch = self._torch
        cap = n_entries if cap is None else int(cap)
        if cap < 0:
            raise ValueError("cap must not be negative")
        work_bytes = int(self._lib.pya_peptidoform_workspace_bytes(n_entries))
        with torch.cuda.device(self.device):
            work = torch.empty(max(work_bytes, 1), dtype=torch.uint8, device=self.device)
            records = torch.empty((cap, 48), dtype=torch.uint8, device=self.device)
            n = torch.empty(2, dtype=torch.int32, device=self.device)
        return work, work_bytes, records, cap, n

    def peptidoforms(self, site_probs, psm_probs, group, threshold=0.75, psm_id=None, psm_base=0, prev=None, cap=None):
        """The peptidoform list of the last ``run()`` (``pya_plan_peptidoforms``): one 48-byte ``pya_peptidoform`` per distinct
        (group, best_sig) among the scored PSMs with a non-negative group, ordered by group, then sig_bits.  ``site_probs`` /
        ``psm_probs``: the two tensors of ``probs()``; ``group``: ``torch.int32`` device tensor ``[n_psm]``; ``psm_id`` /
        ``psm_base`` as for ``rollup()``; ``prev``: the records of an earlier list (``torch.uint8 [n_prev, 48]``, only read) --
        the result is then the list over the PSMs behind both, the bytes of one call over all of them; ``cap``: the room of
        the result (default: PSMs + earlier records, which always suffices).  Returns device tensors ``(records, n)``:
        ``torch.uint8 [cap, 48]`` (``peptidoform_records`` turns a host copy of the first ``n[0]`` into the structured array)
        and ``torch.int32 [2]``: the length of the list and an error word.  The workspace is a torch tensor that lives for
        the call; everything is launched on torch's current stream and nothing waits on the host."""
        torch = self._torch
        n_rec = int(self.site_offsets()[-1])
        if group.dtype != torch.int32 or tuple(group.shape) != (self.n_psm,) or not group.is_contiguous() or not group.is_cuda:
            raise ValueError("group must be a contiguous int32 device tensor of %d entries" % self.n_psm)
        if site_probs.dtype != torch.float64 or tuple(site_probs.shape) != (n_rec, 2) or not site_probs.is_contiguous() or not site_probs.is_cuda \
                or psm_probs.dtype != torch.uint8 or tuple(psm_probs.shape) != (self.n_psm, 16) or not psm_probs.is_contiguous() or not psm_probs.is_cuda:
            raise ValueError("site_probs and psm_probs must be the tensors of probs()")
        if psm_id is not None and (psm_id.element_size() != 4 or psm_id.is_floating_point() or tuple(psm_id.shape) != (self.n_psm,)
                                   or not psm_id.is_contiguous() or not psm_id.is_cuda):
            raise ValueError("psm_id must be a contiguous 32-bit integer device tensor of %d entries" % self.n_psm)
        prev, n_prev = self._pform_records(prev, "prev")
        work, work_bytes, records, cap, n = self._pform_buffers(self.n_psm + n_prev, cap)
        stream = torch.cuda.current_stream(self.device)
        rc = self._lib.pya_plan_peptidoforms(self._plan, C.byref(self._res), stream.cuda_stream, site_probs.data_ptr(), psm_probs.data_ptr(),
                                             group.data_ptr(), float(threshold), None if psm_id is None else psm_id.data_ptr(), int(psm_base),
                                             None if not n_prev else prev.data_ptr(), n_prev, work.data_ptr(), work_bytes,
                                             records.data_ptr(), cap, n.data_ptr())
        if rc:
            self.scorer._raise(rc)
        work.record_stream(stream)                 # (the caching allocator must not hand the workspace on before the stream is past it)
        return records, n

    def peptidoform_reduce(self, a, b=None, cap=None):
        """The list over one or two device arrays of peptidoform records (``torch.uint8 [n, 48]``, any order, keys may repeat,
        records with ``n_psm == 0`` are skipped; ``pya_peptidoform_reduce``): merging two lists is this call.  Returns
        ``(records, n)`` as ``peptidoforms()`` does; the inputs are only read."""
        torch = self._torch
        a, n_a = self._pform_records(a, "a")
        b, n_b = self._pform_records(b, "b")
        work, work_bytes, records, cap, n = self._pform_buffers(n_a + n_b, cap)
        stream = torch.cuda.current_stream(self.device)
        rc = self._lib.pya_peptidoform_reduce(self.scorer._h, None if not n_a else a.data_ptr(), n_a, None if not n_b else b.data_ptr(), n_b,
                                              stream.cuda_stream, work.data_ptr(), work_bytes, records.data_ptr(), cap, n.data_ptr())
        if rc:
            self.scorer._raise(rc)
        work.record_stream(stream)
        return records, n

    def _pfq_table(self, pair, what, n_ch):
        """an input pair ``(records, head, cell)`` (head and cell None: an all-zero table) checked: (records, n, head, cell)"""
        torch = self._torch
        if pair is None:
            return None, 0, None, None
        if len(pair) != 3:
            raise ValueError("%s must be a (records, head, cell) triple" % what)
        records, n = self._pform_records(pair[0], what)
        head, cell = pair[1], pair[2]
        if (head is None) != (cell is None):
            raise ValueError("%s: head and cell are both given or both None" % what)
        if head is not None and (head.dtype != torch.uint8 or tuple(head.shape) != (n, 8) or not head.is_contiguous() or not head.is_cuda
                                 or cell.dtype != torch.uint8 or tuple(cell.shape) != (n, n_ch, 16) or not cell.is_contiguous()
                                 or not cell.is_cuda):
            raise ValueError("%s: the table must be contiguous uint8 device tensors of shapes (%d, 8) and (%d, %d, 16)" % (what, n, n, n_ch))
        return records, n, head, cell

    def _pfq_buffers(self, n_entries, n_ch, cap):
        torch = self._torch
        cap = n_entries if cap is None else int(cap)
        if cap < 0:
            raise ValueError("cap must not be negative")
        work_bytes = int(self._lib.pya_peptidoform_quant_workspace_bytes(n_entries, n_ch))
        with torch.cuda.device(self.device):
            work = torch.empty(max(work_bytes, 1), dtype=torch.uint8, device=self.device)
            records = torch.empty((cap, 48), dtype=torch.uint8, device=self.device)
            head = torch.empty((cap, 8), dtype=torch.uint8, device=self.device)
            cell = torch.empty((cap, n_ch, 16), dtype=torch.uint8, device=self.device)
            n = torch.empty(2, dtype=torch.int32, device=self.device)
        return work, work_bytes, records, head, cell, cap, n

    def peptidoform_quant(self, site_probs, psm_probs, group, values, params, threshold=0.75, psm_id=None, psm_base=0, row=None, row_base=0,
                          prev=None, cap=None):
        """The peptidoform quantification of the last ``run()`` (``pya_plan_peptidoform_quant``): the list ``peptidoforms()``
        gives for the same arguments, byte for byte, and row-aligned with it the channel sums of the PSMs that contribute to
        the list with ``min_prob >= params["threshold"]``.  ``site_probs`` / ``psm_probs`` / ``group`` / ``threshold`` /
        ``psm_id`` / ``psm_base`` as for ``peptidoforms()``; ``values`` / ``params`` / ``row`` / ``row_base`` as for
        ``site_quant()``; ``prev``: an earlier pair ``(records, head, cell)`` of device tensors (only read; head and cell None:
        an all-zero table) -- the result is then the pair over the PSMs behind both; ``cap``: the room of the result.  Returns
        device tensors ``(records, head, cell, n)``: ``torch.uint8 [cap, 48]``, ``[cap, 8]``, ``[cap, n_channels, 16]`` (rows
        behind the list are zero bytes in the table) and ``torch.int32 [2]`` as for ``peptidoforms()``.  Everything is launched
        on torch's current stream and nothing waits on the host; a PSM whose row lies at or above ``n_rows`` writes nothing to
        the table and is reported by ``check()``."""
        from .rollup import site_quant_c_params
        torch = self._torch
        c_params = site_quant_c_params(params)
        n_ch = int(c_params.n_channels)
        n_rec = int(self.site_offsets()[-1])
        if group.dtype != torch.int32 or tuple(group.shape) != (self.n_psm,) or not group.is_contiguous() or not group.is_cuda:
            raise ValueError("group must be a contiguous int32 device tensor of %d entries" % self.n_psm)
        if site_probs.dtype != torch.float64 or tuple(site_probs.shape) != (n_rec, 2) or not site_probs.is_contiguous() or not site_probs.is_cuda \
                or psm_probs.dtype != torch.uint8 or tuple(psm_probs.shape) != (self.n_psm, 16) or not psm_probs.is_contiguous() or not psm_probs.is_cuda:
            raise ValueError("site_probs and psm_probs must be the tensors of probs()")
        if psm_id is not None and (psm_id.element_size() != 4 or psm_id.is_floating_point() or tuple(psm_id.shape) != (self.n_psm,)
                                   or not psm_id.is_contiguous() or not psm_id.is_cuda):
            raise ValueError("psm_id must be a contiguous 32-bit integer device tensor of %d entries" % self.n_psm)
        if values.dtype != torch.float64 or values.dim() != 2 or values.shape[1] != n_ch or not values.is_contiguous() or not values.is_cuda:
            raise ValueError("values must be a contiguous float64 device tensor of shape (n_rows, %d)" % n_ch)
        if row is not None and (row.dtype != torch.int32 or tuple(row.shape) != (self.n_psm,) or not row.is_contiguous() or not row.is_cuda):
            raise ValueError("row must be a contiguous int32 device tensor of %d entries" % self.n_psm)
        prev, n_prev, p_head, p_cell = self._pfq_table(prev, "prev", n_ch)
        work, work_bytes, records, head, cell, cap, n = self._pfq_buffers(self.n_psm + n_prev, n_ch, cap)
        stream = torch.cuda.current_stream(self.device)
        ptr = lambda t: None if t is None or not t.numel() else t.data_ptr()  # noqa: E731
        rc = self._lib.pya_plan_peptidoform_quant(self._plan, C.byref(self._res), stream.cuda_stream, site_probs.data_ptr(), psm_probs.data_ptr(),
                                                  group.data_ptr(), float(threshold), None if psm_id is None else psm_id.data_ptr(),
                                                  int(psm_base), ptr(prev), ptr(p_head), ptr(p_cell), n_prev, ptr(values), values.shape[0],
                                                  None if row is None else row.data_ptr(), int(row_base), C.byref(c_params), work.data_ptr(),
                                                  work_bytes, ptr(records), ptr(head), ptr(cell), cap, n.data_ptr())
        if rc:
            self.scorer._raise(rc)
        work.record_stream(stream)                 # (the caching allocator must not hand the workspace on before the stream is past it)
        return records, head, cell, n

    def peptidoform_quant_reduce(self, a, b=None, n_channels=None, cap=None):
        """The merge of two peptidoform quantification pairs on the device (``pya_peptidoform_quant_reduce``): ``a`` and ``b``
        are ``(records, head, cell)`` triples of device tensors as ``peptidoform_quant()`` returns them cut to their length (any
        order, keys may repeat, records with ``n_psm == 0`` are skipped with their rows; head and cell None: an all-zero table).
        ``n_channels`` is needed only when neither side has a table.  Returns ``(records, head, cell, n)`` as
        ``peptidoform_quant()`` does; the inputs are only read."""
        torch = self._torch
        n_ch = n_channels
        for pair in (a, b):
            if pair is not None and len(pair) == 3 and pair[2] is not None and pair[2].dim() == 3:
                n_ch = int(pair[2].shape[1])
        if n_ch is None:
            raise ValueError("peptidoform_quant_reduce: neither side has a table; pass n_channels")
        ra, n_a, ha, ca = self._pfq_table(a, "a", n_ch)
        rb, n_b, hb, cb = self._pfq_table(b, "b", n_ch)
        work, work_bytes, records, head, cell, cap, n = self._pfq_buffers(n_a + n_b, n_ch, cap)
        stream = torch.cuda.current_stream(self.device)
        ptr = lambda t: None if t is None or not t.numel() else t.data_ptr()  # noqa: E731
        rc = self._lib.pya_peptidoform_quant_reduce(self.scorer._h, ptr(ra), ptr(ha), ptr(ca), n_a, ptr(rb), ptr(hb), ptr(cb), n_b, int(n_ch),
                                                    stream.cuda_stream, work.data_ptr(), work_bytes, ptr(records), ptr(head), ptr(cell), cap,
                                                    n.data_ptr())
        if rc:
            self.scorer._raise(rc)
        work.record_stream(stream)
        return records, head, cell, n

    def mz_profile(self, params, run=None, n_slots=None, table=None):
        """Adds the fragment mass errors of the last ``run()`` to ``table`` (``pya_plan_mz_profile``): a ``torch.uint8`` device
        tensor ``[n_slots, 4128]`` (one ``pya_mz_profile`` per run slot; ``mz_profile_records`` turns a host copy into the
        structured array), new and zeroed when None -- ``n_slots`` of them, 1 by default.  The stage ACCUMULATES: the same
        table takes other plans, runs and calls, and an empty table is all-zero bytes.  ``params``:
        ``pyascore_amd.rollup.mz_profile_params(...)``; ``run``: ``torch.int32`` device tensor ``[n_psm]``, the slot of every
        PSM (negative: left out), or None: slot 0.  One or two launches on torch's current stream; nothing waits on the host.
        A slot at or above the table's size writes nothing and is reported by ``check()``.  Returns ``table``."""
        torch = self._torch
        if table is None:
            with torch.cuda.device(self.device):
                table = torch.zeros((1 if n_slots is None else int(n_slots), MZ_PROFILE_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != MZ_PROFILE_DTYPE.itemsize or not table.is_contiguous() \
                or not table.is_cuda:
            raise ValueError("table must be a contiguous uint8 device tensor of shape (n_slots, %d)" % MZ_PROFILE_DTYPE.itemsize)
        if run is not None and (run.dtype != torch.int32 or tuple(run.shape) != (self.n_psm,) or not run.is_contiguous() or not run.is_cuda):
            raise ValueError("run must be a contiguous int32 device tensor of %d entries" % self.n_psm)
        c_params = _lib.MzProfileParams(params["inv_da"], params["inv_ppm"], params["inv_band"], params["max_rank"], 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.pya_plan_mz_profile(self._plan, C.byref(self._res), stream, None if run is None else run.data_ptr(), table.shape[0],
                                           C.byref(c_params), table.data_ptr())
        if rc:
            self.scorer._raise(rc)
        return table

    def coverage(self, d_mz, d_intensity, out=None):
        """The coverage records of the last ``run()`` as a ``torch.uint8`` device tensor ``[n_psm, 64]`` (one ``pya_coverage``
        per PSM; ``coverage_records`` turns a host copy into the structured array).  ``d_mz`` / ``d_intensity``: the tensors
        that run was given -- the stage reads the raw peaks again.  One or two launches on torch's current stream; nothing
        waits on the host.  Returns ``out`` (every byte of it is written)."""
        torch = self._torch
        for t in (d_mz, d_intensity):
            if t.dtype not in (torch.float64, torch.float32) or not t.is_cuda or not t.is_contiguous():
                raise ValueError("spectra must be the contiguous device tensors the plan was run with")
        shape = (self.n_psm, COVERAGE_DTYPE.itemsize)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous uint8 device tensor of shape %r" % (shape,))
        sp = _lib.TypedSpectra(d_mz.data_ptr(), d_intensity.data_ptr(), _lib.spectrum_type(d_mz.dtype), _lib.spectrum_type(d_intensity.dtype))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.pya_plan_coverage(self._plan, C.byref(self._res), C.byref(sp), stream, out.data_ptr())
        if rc:
            self.scorer._raise(rc)
        return out

    def fit_mz_calibration(self, table, params, min_ions=20, out=None):
        """The m/z calibration of a profile ``table`` (the ``torch.uint8`` device tensor ``[n_slots, 4128]`` of ``mz_profile()``)
        as a ``torch.uint8`` device tensor ``[n_slots, 128]``, one ``pya_mz_calibration`` per slot (``pya_mz_profile_fit``;
        ``mz_calibration_records`` turns a host copy into the structured array).  ``params``: the ``mz_profile_params`` the
        table was binned with; ``min_ions``: the signal ions a band needs to be fitted.  One launch on torch's current stream;
        nothing waits on the host.  Returns ``out`` (every byte of it is written)."""
        torch = self._torch
        if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != MZ_PROFILE_DTYPE.itemsize or not table.is_contiguous() \
                or not table.is_cuda:
            raise ValueError("table must be a contiguous uint8 device tensor of shape (n_slots, %d)" % MZ_PROFILE_DTYPE.itemsize)
        shape = (table.shape[0], MZ_CALIBRATION_DTYPE.itemsize)
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous uint8 device tensor of shape %r" % (shape,))
        c_params = _lib.MzProfileParams(params["inv_da"], params["inv_ppm"], params["inv_band"], params["max_rank"], 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.pya_mz_profile_fit(self.scorer._h, table.data_ptr(), table.shape[0], C.byref(c_params), int(min_ions), stream,
                                          out.data_ptr())
        if rc:
            self.scorer._raise(rc)
        return out

    def recalibrate(self, d_mz, peak_off, cal, run=None, band_width=250.0, out=None):
        """Corrects the m/z tensor of spectra with a calibration on the device (``pya_recalibrate_spectra``): ``d_mz`` a
        contiguous float64 or float32 device tensor, ``peak_off`` an ``int64`` device tensor ``[n_spectra + 1]``, ``cal`` the
        ``torch.uint8`` device tensor ``[n_slots, 128]`` of ``fit_mz_calibration()``, ``run`` an ``int32`` device tensor
        ``[n_spectra]`` with the slot of every spectrum (negative: left as it is) or None: slot 0, ``band_width`` the width of
        the bands the calibration was fitted over.  ``out``: a tensor like ``d_mz`` -- ``d_mz`` itself corrects in place --, new
        when None.  One launch on torch's current stream; nothing waits on the host.  ``pyascore_amd.rollup.recalibrate`` gives
        the same bytes.  A spectrum whose slot is outside ``cal`` or whose record has a knot that is not finite or beyond 1000 ppm
        is copied unchanged and counted in ``last_recalibrate_over`` (an ``int32`` device tensor of two words: the count, and
        0xffffffff minus the first such spectrum).  Returns ``out``."""
        torch = self._torch
        if d_mz.dtype not in (torch.float64, torch.float32) or not d_mz.is_cuda or not d_mz.is_contiguous() or d_mz.dim() != 1:
            raise ValueError("d_mz must be a contiguous one-dimensional float64 or float32 device tensor")
        if peak_off.dtype != torch.int64 or peak_off.dim() != 1 or peak_off.numel() < 1 or not peak_off.is_contiguous() or not peak_off.is_cuda:
            raise ValueError("peak_off must be a contiguous int64 device tensor of n_spectra + 1 entries")
        n_spec = peak_off.numel() - 1
        if cal.dtype != torch.uint8 or cal.dim() != 2 or cal.shape[1] != MZ_CALIBRATION_DTYPE.itemsize or not cal.is_contiguous() or not cal.is_cuda:
            raise ValueError("cal must be a contiguous uint8 device tensor of shape (n_slots, %d)" % MZ_CALIBRATION_DTYPE.itemsize)
        if run is not None and (run.dtype != torch.int32 or tuple(run.shape) != (n_spec,) or not run.is_contiguous() or not run.is_cuda):
            raise ValueError("run must be a contiguous int32 device tensor of %d entries" % n_spec)
        if out is None:
            out = torch.empty_like(d_mz)
        if out.dtype != d_mz.dtype or tuple(out.shape) != tuple(d_mz.shape) or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous device tensor of the dtype and shape of d_mz")
        band_width = float(band_width)
        inv_band = 1.0 / band_width if band_width else float("inf")
        with torch.cuda.device(self.device):
            self.last_recalibrate_over = torch.zeros(2, dtype=torch.int32, device=self.device)
        sp = _lib.TypedSpectra(d_mz.data_ptr(), None, _lib.spectrum_type(d_mz.dtype), _lib.PYA_F64)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.pya_recalibrate_spectra(self.scorer._h, C.byref(sp), peak_off.data_ptr(), n_spec, None if run is None else run.data_ptr(),
                                               cal.data_ptr(), cal.shape[0], inv_band, stream, out.data_ptr(),
                                               self.last_recalibrate_over.data_ptr())
        if rc:
            self.scorer._raise(rc)
        return out

    def timings_ms(self):
        """(bin_spectra, score_signatures, score_localize, localize) kernel-family durations of the
        last run; synchronises."""
        ms = (C.c_float * 4)()
        rc = self._lib.pya_plan_timings(self._plan, C.byref(ms))
        if rc:
            self.scorer._raise(rc)
        return tuple(float(x) for x in ms)

    def timings_sum(self):
        """((bin_spectra, score_signatures, score_localize, localize) durations in ms summed over the runs since
        the last call, number of runs).  The events sit in a ring of 128 runs; synchronises with the latest run
        only, so runs can be enqueued back to back and read afterwards."""
        ms = (C.c_double * 4)()
        n = C.c_uint32(0)
        rc = self._lib.pya_plan_timings_sum(self._plan, C.byref(ms), C.byref(n))
        if rc:
            self.scorer._raise(rc)
        return tuple(float(x) for x in ms), int(n.value)

    def check(self):
        rc = self._lib.pya_plan_check(self._plan)
        if rc:
            self.scorer._raise(rc)

    def packed_summary(self, out=None):
        """Results as one [n_psm, 4 + 3*max_k] int32 device tensor (fixed-size records for the
        gather): best_score bits, n_sig, best_sig lo/hi, then per site ascore bits, alt lo/hi.
        ``out``: a preallocated contiguous [n_psm, width] int32 tensor (e.g. a slice of the send buffer).  ONE kernel
        of the library (pya_pack_records) on torch's current stream writes the records in place: no framework kernel
        and no intermediate tensor inside the step (r05: torch.cat)."""
        torch = self._torch
        width = 4 + 3 * self.max_k
        if out is None:
            out = torch.empty((self.n_psm, width), dtype=torch.int32, device=self.device)
        if out.dtype != torch.int32 or tuple(out.shape) != (self.n_psm, width) or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous int32 device tensor of shape (%d, %d)" % (self.n_psm, width))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.pya_pack_records(self.scorer._h, C.byref(self._res), self.n_psm, self.max_k, out.data_ptr(), stream)
        if rc:
            self.scorer._raise(rc)
        return out


EVIDENCE_DTYPE = np.dtype(_lib.EVIDENCE_DTYPE)
ION_DTYPE = np.dtype(_lib.ION_DTYPE)
NAMED_DTYPE = np.dtype(_lib.NAMED_DTYPE)
SITE_DTYPE = np.dtype(_lib.SITE_DTYPE)
PSM_PROB_DTYPE = np.dtype(_lib.PSM_PROB_DTYPE)
RANKED_DTYPE = np.dtype(_lib.RANKED_DTYPE)
ROLLUP_DTYPE = np.dtype(_lib.ROLLUP_DTYPE)
FLR_DTYPE = np.dtype(_lib.FLR_DTYPE)
PEPTIDOFORM_DTYPE = np.dtype(_lib.PEPTIDOFORM_DTYPE)
MZ_PROFILE_DTYPE = np.dtype(_lib.MZ_PROFILE_DTYPE)
MZ_CALIBRATION_DTYPE = np.dtype(_lib.MZ_CALIBRATION_DTYPE)
COVERAGE_DTYPE = np.dtype(_lib.COVERAGE_DTYPE)


def _upload(a, dtype, device):
    """a host array as a contiguous device tensor of ``dtype``"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)


def _transform_inputs(scorer, c_params_of, params, d_mz, d_intensity, peak_off):
    """What ``deisotope``, ``decharge``, ``strip`` and ``centroid`` check alike about what they read: the scorer, ``params``
    (through the stage's ``*_c_params``), the spectrum tensors and ``peak_off`` (a host array is uploaded).  Returns
    ``(c_params, device, peak_off, n_spec)``."""
    import torch
    if not isinstance(scorer, PyAscore):
        raise TypeError("scorer must be a pyascore_amd.PyAscore")
    c_params = c_params_of(params)
    device = torch.device("cuda", scorer.device)
    for t in (d_mz, d_intensity):
        if t.dtype not in (torch.float64, torch.float32) or not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
            raise ValueError("spectra must be contiguous one-dimensional float64 or float32 device tensors")
    if d_mz.dtype == torch.float32 and d_intensity.dtype == torch.float64:
        raise ValueError("float32 m/z beside float64 intensities is not supported")
    if d_mz.numel() != d_intensity.numel():
        raise ValueError("d_mz and d_intensity have one element per peak each")
    if not isinstance(peak_off, torch.Tensor):
        host_off = np.ascontiguousarray(peak_off, np.int64)
        if host_off.ndim != 1 or host_off.size < 1 or int(host_off[-1]) > d_mz.numel():
            raise ValueError("peak_off has n_spectra + 1 entries and ends inside the spectrum tensors")
        peak_off = _upload(host_off, np.int64, device)
    if peak_off.dtype != torch.int64 or peak_off.dim() != 1 or peak_off.numel() < 1 or not peak_off.is_contiguous() or not peak_off.is_cuda:
        raise ValueError("peak_off must be a contiguous int64 tensor of n_spectra + 1 entries")
    return c_params, device, peak_off, peak_off.numel() - 1


def _transform_outputs(workspace_bytes, device, d_mz, d_intensity, n_spec, out, side_shape=None):
    """What they make alike for what they write: ``out`` checked (new when None), the workspace the stage's
    ``pya_*_workspace_bytes`` asks for, the offsets, the two zeroed words of ``d_over`` and, with ``side_shape``, a ``uint8``
    tensor of that shape.  Returns ``(o_mz, o_it, t_in, t_out, stream, work, new_off, over, side)``: the two ``TypedSpectra`` of
    the call and torch's current stream among them."""
    import torch
    if out is None:
        out = (torch.empty_like(d_mz), torch.empty_like(d_intensity))
    o_mz, o_it = out
    for o, t in ((o_mz, d_mz), (o_it, d_intensity)):
        if o.dtype != t.dtype or tuple(o.shape) != tuple(t.shape) or not o.is_contiguous() or not o.is_cuda:
            raise ValueError("out must be a pair of contiguous device tensors of the dtypes and shapes of the inputs")
    with torch.cuda.device(device):
        work = torch.empty((int(workspace_bytes(n_spec, d_mz.numel())) + 7) // 8, dtype=torch.int64, device=device)
        new_off = torch.empty(n_spec + 1, dtype=torch.int64, device=device)
        over = torch.zeros(2, dtype=torch.int32, device=device)
        side = None if side_shape is None else torch.empty(side_shape, dtype=torch.uint8, device=device)
    t_in = _lib.TypedSpectra(d_mz.data_ptr(), d_intensity.data_ptr(), _lib.spectrum_type(d_mz.dtype), _lib.spectrum_type(d_intensity.dtype))
    t_out = _lib.TypedSpectra(o_mz.data_ptr(), o_it.data_ptr(), t_in.mz_type, t_in.intensity_type)
    return o_mz, o_it, t_in, t_out, torch.cuda.current_stream(device).cuda_stream, work, new_off, over, side


def deisotope(scorer, d_mz, d_intensity, peak_off, params, out=None):
    """Deisotopes spectra that live on the device (``pya_deisotope_spectra``; the rule is ``pya_deisotope_params``'s in
    include/pyascore_hip.h): ``d_mz`` / ``d_intensity`` contiguous float64 or float32 device tensors (float64 / float64, float64
    m/z with float32 intensities, or both float32), ``peak_off`` an ``int64`` tensor or array ``[n_spectra + 1]`` (a host array
    is uploaded), ``params`` of ``pyascore_amd.rollup.deisotope_params``.  ``out``: a pair of tensors like the inputs to write
    into (not the inputs themselves), new when None.  Returns ``(d_mz_out, d_intensity_out, d_new_off, d_over)``: the kept peaks
    of spectrum s are ``out[d_new_off[s]:d_new_off[s + 1]]`` bit for bit, the elements from ``d_new_off[-1]`` on are not
    written; ``d_over`` is an ``int32`` tensor of two words (the spectra that were not ascending and were copied, and
    0xffffffff minus the first of them).  Three launches on torch's current stream; nothing waits on the host.  A plan needs
    the peak counts on the host: read ``d_new_off`` back and build the ``DevicePlan`` with it as ``peak_off``.
    ``pyascore_amd.rollup.deisotope`` gives the same bytes."""
    from .rollup import deisotope_c_params
    c_params, device, peak_off, n_spec = _transform_inputs(scorer, deisotope_c_params, params, d_mz, d_intensity, peak_off)
    o_mz, o_it, t_in, t_out, stream, work, new_off, over, _ = _transform_outputs(
        scorer._lib.pya_deisotope_workspace_bytes, device, d_mz, d_intensity, n_spec, out)
    rc = scorer._lib.pya_deisotope_spectra(scorer._h, C.byref(t_in), peak_off.data_ptr(), n_spec, C.byref(c_params), stream, work.data_ptr(),
                                           work.numel() * 8, C.byref(t_out), new_off.data_ptr(), over.data_ptr())
    if rc:
        scorer._raise(rc)
    # (the caching allocator keeps `work` for this stream until later work on the stream is done with it)
    return o_mz, o_it, new_off, over


def decharge(scorer, d_mz, d_intensity, peak_off, params, out=None, charge=True):
    """Charge-deconvolves spectra that live on the device (``pya_decharge_spectra``; the rule is ``pya_decharge_params``'s in
    include/pyascore_hip.h): arguments as ``deisotope`` takes them, ``params`` of ``pyascore_amd.rollup.decharge_params``;
    ``charge=False`` leaves the charges out (``d_charge = NULL``).  Returns ``(d_mz_out, d_intensity_out, d_new_off, d_charge,
    d_over)``: the peaks of spectrum s are ``out[d_new_off[s]:d_new_off[s + 1]]``, ascending, the elements from
    ``d_new_off[-1]`` on are not written; ``d_charge`` is a ``uint8`` tensor of the inputs' length with the charge of every
    output peak (1: not moved), or None; ``d_over`` as ``deisotope`` returns it.  Three launches on torch's current stream;
    nothing waits on the host.  A plan needs the peak counts on the host: read ``d_new_off`` back and build the ``DevicePlan``
    with it as ``peak_off``; leave ``max_fragment_charge`` at 1.  ``pyascore_amd.rollup.decharge`` gives the same bytes."""
    from .rollup import decharge_c_params
    c_params, device, peak_off, n_spec = _transform_inputs(scorer, decharge_c_params, params, d_mz, d_intensity, peak_off)
    o_mz, o_it, t_in, t_out, stream, work, new_off, over, d_charge = _transform_outputs(
        scorer._lib.pya_decharge_workspace_bytes, device, d_mz, d_intensity, n_spec, out, (d_mz.numel(),) if charge else None)
    rc = scorer._lib.pya_decharge_spectra(scorer._h, C.byref(t_in), peak_off.data_ptr(), n_spec, C.byref(c_params), stream, work.data_ptr(),
                                          work.numel() * 8, C.byref(t_out), new_off.data_ptr(),
                                          d_charge.data_ptr() if charge and d_charge.numel() else None, over.data_ptr())
    if rc:
        scorer._raise(rc)
    # (the caching allocator keeps `work` for this stream until later work on the stream is done with it)
    return o_mz, o_it, new_off, d_charge, over


def strip(scorer, d_mz, d_intensity, peak_off, d_prec_mz, d_prec_z, params, out=None, report=True):
    """Strips the precursor-derived peaks from spectra that live on the device (``pya_strip_spectra``; the rule is
    ``pya_strip_params``'s in include/pyascore_hip.h): spectra, ``peak_off`` and ``out`` as ``deisotope`` takes them,
    ``d_prec_mz`` / ``d_prec_z`` the precursor m/z (float64) and charge (int32) of every spectrum as device tensors or host
    arrays (a host array is uploaded), ``params`` of ``pyascore_amd.rollup.strip_params``; ``report=False`` leaves the report
    out (``d_report = NULL``).  Returns ``(d_mz_out, d_intensity_out, d_new_off, d_report, d_over)``: the kept peaks of spectrum
    s are ``out[d_new_off[s]:d_new_off[s + 1]]`` bit for bit, the elements from ``d_new_off[-1]`` on are not written;
    ``d_report`` is a ``uint8`` tensor ``[n_spectra, 16]`` (``.cpu().numpy().view(pyascore_amd.rollup.STRIP_REPORT_DTYPE)``),
    or None; ``d_over`` as ``deisotope`` returns it (two zeros: the workspace is sized here).  Three launches on torch's current
    stream; nothing waits on the host.  A plan needs the peak counts on the host: read ``d_new_off`` back and build the
    ``DevicePlan`` with it as ``peak_off``; ``deisotope`` / ``decharge`` take the outputs as they are, with ``d_new_off`` as
    their ``peak_off``.  ``pyascore_amd.rollup.strip`` gives the same bytes."""
    import torch
    from .rollup import strip_c_params
    c_params, device, peak_off, n_spec = _transform_inputs(scorer, strip_c_params, params, d_mz, d_intensity, peak_off)
    if not isinstance(d_prec_mz, torch.Tensor):
        d_prec_mz = _upload(d_prec_mz, np.float64, device)
    if not isinstance(d_prec_z, torch.Tensor):
        d_prec_z = _upload(d_prec_z, np.int32, device)
    for t, dtype in ((d_prec_mz, torch.float64), (d_prec_z, torch.int32)):
        if t.dtype != dtype or tuple(t.shape) != (n_spec,) or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("d_prec_mz (float64) and d_prec_z (int32) are contiguous device tensors with one entry per spectrum")
    o_mz, o_it, t_in, t_out, stream, work, new_off, over, d_report = _transform_outputs(
        scorer._lib.pya_strip_workspace_bytes, device, d_mz, d_intensity, n_spec, out, (n_spec, 16) if report else None)
    rc = scorer._lib.pya_strip_spectra(scorer._h, C.byref(t_in), peak_off.data_ptr(), n_spec, d_prec_mz.data_ptr(), d_prec_z.data_ptr(),
                                       C.byref(c_params), stream, work.data_ptr(), work.numel() * 8, C.byref(t_out), new_off.data_ptr(),
                                       d_report.data_ptr() if report and n_spec else None, over.data_ptr())
    if rc:
        scorer._raise(rc)
    # (the caching allocator keeps `work` for this stream until later work on the stream is done with it)
    return o_mz, o_it, new_off, d_report, over


def centroid(scorer, d_mz, d_intensity, peak_off, params, select=None, out=None):
    """Centroids profile-mode spectra that live on the device (``pya_centroid_spectra``; the rule is ``pya_centroid_params``'s
    in include/pyascore_hip.h): spectra, ``peak_off`` and ``out`` as ``deisotope`` takes them, ``params`` of
    ``pyascore_amd.rollup.centroid_params``, ``select`` one byte per spectrum as a ``uint8`` / ``bool`` device tensor or a
    host array (uploaded; 0: the spectrum is copied unchanged) or None for all.  Returns ``(d_mz_out, d_intensity_out,
    d_new_off, d_over)``: the peaks of spectrum s are ``out[d_new_off[s]:d_new_off[s + 1]]``, one per apex, the elements from
    ``d_new_off[-1]`` on are not written; ``d_over`` as ``deisotope`` returns it (the selected spectra that were not ascending
    and were copied).  Three launches on torch's current stream; nothing waits on the host.  The first of the transforms:
    ``strip`` / ``deisotope`` / ``decharge`` take the outputs as they are, with ``d_new_off`` as their ``peak_off``; a plan
    needs the peak counts on the host.  ``pyascore_amd.rollup.centroid`` gives the same bytes."""
    import torch
    from .rollup import centroid_c_params, centroid_select
    c_params, device, peak_off, n_spec = _transform_inputs(scorer, centroid_c_params, params, d_mz, d_intensity, peak_off)
    if select is not None and not isinstance(select, torch.Tensor):
        select = _upload(centroid_select(select, n_spec, "centroid"), np.uint8, device)
    if select is not None:
        if select.dtype not in (torch.uint8, torch.bool) or tuple(select.shape) != (n_spec,) or not select.is_contiguous() or not select.is_cuda:
            raise ValueError("select is a contiguous uint8 or bool device tensor with one entry per spectrum")
    o_mz, o_it, t_in, t_out, stream, work, new_off, over, _ = _transform_outputs(
        scorer._lib.pya_centroid_workspace_bytes, device, d_mz, d_intensity, n_spec, out)
    rc = scorer._lib.pya_centroid_spectra(scorer._h, C.byref(t_in), peak_off.data_ptr(), n_spec,
                                          select.data_ptr() if select is not None and n_spec else None, C.byref(c_params), stream,
                                          work.data_ptr(), work.numel() * 8, C.byref(t_out), new_off.data_ptr(), over.data_ptr())
    if rc:
        scorer._raise(rc)
    # (the caching allocator keeps `work` and `select` for this stream until later work on the stream is done with them)
    return o_mz, o_it, new_off, over


def markers(scorer, d_mz, d_intensity, peak_off, params, d_prec_mz=None, d_prec_z=None, out=None):
    """Looks up the marker ions of spectra that live on the device (``pya_marker_spectra``; the rule is ``pya_marker_params``'s
    in include/pyascore_hip.h): spectra and ``peak_off`` as ``deisotope`` takes them, ``params`` of
    ``pyascore_amd.rollup.marker_params``, ``d_prec_mz`` / ``d_prec_z`` the precursor m/z (float64) and charge (int32) of every
    spectrum as device tensors or host arrays (a host array is uploaded), needed iff ``params`` has loss targets.  ``out``: a
    pair of contiguous ``uint8`` device tensors ``[n_spectra, n_targets, 24]`` and ``[n_spectra, 32]`` to write into, new when
    None.  Returns ``(d_markers, d_spectra, d_over)``: the two record tensors (``marker_records`` / ``marker_spectrum_records``
    read host copies of them) and ``d_over`` as ``deisotope`` returns it (the spectra whose offsets reach beyond the tensors).
    READ-ONLY: the spectra are not written and nothing needs the result on the host, so the call sits anywhere in a chain of
    device forms -- in front of ``strip``, to see the peaks it cuts.  One launch on torch's current stream; nothing waits on
    the host.  ``pyascore_amd.rollup.markers`` gives the same bytes."""
    import torch
    from .rollup import MARKER_DTYPE, MARKER_SPECTRUM_DTYPE, marker_c_params
    c_params, device, peak_off, n_spec = _transform_inputs(scorer, marker_c_params, params, d_mz, d_intensity, peak_off)
    if (d_prec_mz is None) != (d_prec_z is None) or (d_prec_mz is None and c_params.loss_mask):
        raise ValueError("d_prec_mz and d_prec_z come together, and loss targets need both")
    if d_prec_mz is not None:
        if not isinstance(d_prec_mz, torch.Tensor):
            d_prec_mz = _upload(d_prec_mz, np.float64, device)
        if not isinstance(d_prec_z, torch.Tensor):
            d_prec_z = _upload(d_prec_z, np.int32, device)
        for t, dtype in ((d_prec_mz, torch.float64), (d_prec_z, torch.int32)):
            if t.dtype != dtype or tuple(t.shape) != (n_spec,) or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("d_prec_mz (float64) and d_prec_z (int32) are contiguous device tensors with one entry per spectrum")
    shapes = (n_spec, int(c_params.n_targets), MARKER_DTYPE.itemsize), (n_spec, MARKER_SPECTRUM_DTYPE.itemsize)
    with torch.cuda.device(device):
        if out is None:
            out = tuple(torch.empty(shape, dtype=torch.uint8, device=device) for shape in shapes)
        over = torch.zeros(2, dtype=torch.int32, device=device)
    d_markers, d_spectra = out
    for o, shape in zip(out, shapes):
        if o.dtype != torch.uint8 or tuple(o.shape) != shape or not o.is_contiguous() or not o.is_cuda:
            raise ValueError("out must be a pair of contiguous uint8 device tensors of shapes %r and %r" % shapes)
    t_in = _lib.TypedSpectra(d_mz.data_ptr(), d_intensity.data_ptr(), _lib.spectrum_type(d_mz.dtype), _lib.spectrum_type(d_intensity.dtype))
    rc = scorer._lib.pya_marker_spectra(scorer._h, C.byref(t_in), peak_off.data_ptr(), n_spec, d_mz.numel(),
                                        None if d_prec_mz is None or not n_spec else d_prec_mz.data_ptr(),
                                        None if d_prec_z is None or not n_spec else d_prec_z.data_ptr(), C.byref(c_params),
                                        torch.cuda.current_stream(device).cuda_stream, d_markers.data_ptr() if n_spec else None,
                                        d_spectra.data_ptr() if n_spec else None, over.data_ptr())
    if rc:
        scorer._raise(rc)
    # (the caching allocator keeps uploaded precursors for this stream until later work on the stream is done with them)
    return d_markers, d_spectra, over


def marker_values(scorer, d_markers, channel_mask=None, out=None):
    """Marker records that live on the device as the channel matrix ``DevicePlan.site_quant`` takes (``pya_marker_values``):
    ``d_markers`` the first tensor of ``markers`` (uint8 ``[n_spectra, n_targets, 24]``), ``channel_mask`` an integer with one
    bit per target that becomes a channel (None: every target), in ascending order.  Returns a ``torch.float64`` device tensor
    ``[n_spectra, popcount(channel_mask)]``: the picked intensity, NaN where the target picked no peak -- the columns of
    ``pyascore_amd.rollup.marker_matrix`` the mask names, with the same bytes.  ``out``: such a tensor to write into.  One launch
    on torch's current stream; nothing waits on the host."""
    import torch
    from .rollup import MARKER_DTYPE
    if not isinstance(scorer, PyAscore):
        raise TypeError("scorer must be a pyascore_amd.PyAscore")
    if d_markers.dtype != torch.uint8 or d_markers.dim() != 3 or d_markers.shape[2] != MARKER_DTYPE.itemsize or not d_markers.is_contiguous() \
            or not d_markers.is_cuda:
        raise ValueError("d_markers must be a contiguous uint8 device tensor of shape (n_spectra, n_targets, %d)" % MARKER_DTYPE.itemsize)
    n_spec, n_t = int(d_markers.shape[0]), int(d_markers.shape[1])
    mask = (1 << n_t) - 1 if channel_mask is None else int(channel_mask)
    if not 1 <= n_t <= 64 or mask <= 0 or mask >> n_t:
        raise ValueError("channel_mask must name at least one of the %d targets and none beyond them" % n_t)
    shape = (n_spec, bin(mask).count("1"))
    device = d_markers.device
    if out is None:
        with torch.cuda.device(device):
            out = torch.empty(shape, dtype=torch.float64, device=device)
    if out.dtype != torch.float64 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous float64 device tensor of shape %r" % (shape,))
    rc = scorer._lib.pya_marker_values(scorer._h, d_markers.data_ptr() if n_spec else None, n_spec, n_t, mask,
                                       torch.cuda.current_stream(device).cuda_stream, out.data_ptr() if n_spec else None)
    if rc:
        scorer._raise(rc)
    return out


def purity(scorer, d_ms1_mz, d_ms1_intensity, ms1_peak_off, d_survey, d_prec_mz, d_prec_z, d_win_lo, d_win_hi, params, out=None):
    """The precursor purity of isolation windows over survey spectra that live on the device (``pya_purity_spectra``; the rule
    is ``pya_purity_params``'s in include/pyascore_hip.h): ``d_ms1_mz`` / ``d_ms1_intensity`` / ``ms1_peak_off`` the survey
    (MS1) spectra as ``deisotope`` takes spectra; ``d_survey`` (int64), ``d_prec_mz`` (float64), ``d_prec_z`` (int32),
    ``d_win_lo`` / ``d_win_hi`` (float64) one entry per query as device tensors or host arrays (a host array is uploaded);
    ``params`` of ``pyascore_amd.rollup.purity_params``.  ``out``: a contiguous ``uint8`` device tensor ``[n_query, 48]`` to write
    into, new when None.  Returns ``(d_purity, d_over)``: the records (``purity_records`` reads a host copy) and an ``int32``
    tensor of two words (the queries whose survey index lies beyond the survey spectra, and 0xffffffff minus the first of
    them).  READ-ONLY; one launch on torch's current stream; nothing waits on the host.  ``pyascore_amd.rollup.purity`` gives
    the same bytes."""
    import torch
    from .rollup import PURITY_DTYPE, purity_c_params
    c_params, device, peak_off, n_survey = _transform_inputs(scorer, purity_c_params, params, d_ms1_mz, d_ms1_intensity, ms1_peak_off)
    per_query = []
    for t, np_dtype, dtype in ((d_survey, np.int64, torch.int64), (d_prec_mz, np.float64, torch.float64), (d_prec_z, np.int32, torch.int32),
                               (d_win_lo, np.float64, torch.float64), (d_win_hi, np.float64, torch.float64)):
        if not isinstance(t, torch.Tensor):
            t = _upload(t, np_dtype, device)
        if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda or (per_query and t.numel() != per_query[0].numel()):
            raise ValueError("d_survey (int64), d_prec_mz (float64), d_prec_z (int32), d_win_lo and d_win_hi (float64) are contiguous "
                             "device tensors with one entry per query")
        per_query.append(t)
    n_query = per_query[0].numel()
    shape = (n_query, PURITY_DTYPE.itemsize)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=device)
        over = torch.zeros(2, dtype=torch.int32, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous uint8 device tensor of shape %r" % (shape,))
    t_in = _lib.TypedSpectra(d_ms1_mz.data_ptr(), d_ms1_intensity.data_ptr(), _lib.spectrum_type(d_ms1_mz.dtype),
                             _lib.spectrum_type(d_ms1_intensity.dtype))
    rc = scorer._lib.pya_purity_spectra(scorer._h, C.byref(t_in), peak_off.data_ptr(), n_survey, d_ms1_mz.numel(),
                                        *(t.data_ptr() if n_query else None for t in per_query), n_query, C.byref(c_params),
                                        torch.cuda.current_stream(device).cuda_stream, out.data_ptr() if n_query else None, over.data_ptr())
    if rc:
        scorer._raise(rc)
    # (the caching allocator keeps uploaded queries for this stream until later work on the stream is done with them)
    return out, over


def purity_gate(scorer, d_purity, threshold, keep_unknown=True, d_values=None, out=None, select=False):
    """THE GATE of the precursor purity over records that live on the device (``pya_purity_gate``): ``d_purity`` the tensor of
    ``purity`` (uint8 ``[n_rows, 48]``), ``threshold`` in 0 .. 1, ``d_values`` a contiguous ``torch.float64`` device tensor
    ``[n_rows, n_channels]`` (what ``marker_values`` returns) or None.  ``out``: such a tensor to write into -- it may be
    ``d_values`` itself: in place --, new when None.  ``select``: True for a new ``uint8`` tensor ``[n_rows]``, or such a tensor,
    to take 1 / 0 per row (what ``channel_sums(select=)`` takes); False: none.  Returns ``(out, select)``, None where not asked
    for: the readings of a passing row copied bit for bit, those of a failing row NaN.  One launch on torch's current stream;
    nothing waits on the host.  ``pyascore_amd.rollup.purity_gate`` gives the same bytes."""
    import torch
    from .rollup import PURITY_DTYPE, check_purity_gate
    if not isinstance(scorer, PyAscore):
        raise TypeError("scorer must be a pyascore_amd.PyAscore")
    t, keep = check_purity_gate(threshold, keep_unknown)
    if d_purity.dim() != 2 or d_purity.shape[1] != PURITY_DTYPE.itemsize:
        raise ValueError("d_purity must be a contiguous uint8 device tensor of shape (n_rows, %d)" % PURITY_DTYPE.itemsize)
    _channel_tensor(d_purity, None, torch.uint8, "d_purity")
    n_rows = int(d_purity.shape[0])
    device = d_purity.device
    n_ch = 0
    if d_values is not None:
        if d_values.dim() != 2 or d_values.shape[0] != n_rows or not 1 <= d_values.shape[1] <= 64:
            raise ValueError("d_values must be a float64 device tensor of shape (n_rows, n_channels), n_channels in 1 .. 64")
        _channel_tensor(d_values, None, torch.float64, "d_values")
        n_ch = int(d_values.shape[1])
        if out is None:
            with torch.cuda.device(device):
                out = torch.empty((n_rows, n_ch), dtype=torch.float64, device=device)
        _channel_tensor(out, (n_rows, n_ch), torch.float64, "out")
    elif out is not None:
        raise ValueError("out goes with d_values")
    if select is True:
        with torch.cuda.device(device):
            select = torch.empty(n_rows, dtype=torch.uint8, device=device)
    elif select is False or select is None:
        select = None
    if select is not None:
        _channel_tensor(select, (n_rows,), torch.uint8, "select")
    if d_values is None and select is None:
        raise ValueError("purity_gate: neither d_values nor select")
    if not n_rows:                                           # (an empty tensor may have no address to pass)
        return out, select
    rc = scorer._lib.pya_purity_gate(scorer._h, d_purity.data_ptr(), n_rows, t, 1 if keep else 0, d_values.data_ptr() if n_ch else None, n_ch,
                                     out.data_ptr() if n_ch else None, None if select is None else select.data_ptr(),
                                     torch.cuda.current_stream(device).cuda_stream)
    if rc:
        scorer._raise(rc)
    return out, select


def _channel_tensor(t, shape, dtype, what):
    if t.dtype != dtype or (shape is not None and tuple(t.shape) != shape) or not t.is_contiguous() or not t.is_cuda:
        raise ValueError("%s must be a contiguous %s device tensor%s" % (what, str(dtype).replace("torch.", ""),
                                                                         "" if shape is None else " of shape %r" % (shape,)))
    return t


def correct_channels(scorer, d_values, matrix=None, factor=None, out=None):
    """APPLY of the channel correction on a matrix that lives on the device (``pya_channel_correct``; the rule is in
    include/pyascore_hip.h): ``d_values`` a contiguous ``torch.float64`` device tensor ``[n_rows, n_channels]`` (what
    ``marker_values`` returns), ``matrix`` ``[n_channels, n_channels]`` and ``factor`` ``[n_channels]`` float64 device tensors or
    host arrays (a host array is uploaded) or None, not both None.  ``out``: such a tensor as ``d_values`` to write into -- it
    may be ``d_values`` itself: in place --, new when None.  Returns it.  One launch on torch's current stream; nothing waits on
    the host.  ``pyascore_amd.rollup.correct_channels`` gives the same bytes."""
    import torch
    if not isinstance(scorer, PyAscore):
        raise TypeError("scorer must be a pyascore_amd.PyAscore")
    if d_values.dim() != 2 or not 1 <= d_values.shape[1] <= 64:
        raise ValueError("d_values must be a float64 device tensor of shape (n_rows, n_channels), n_channels in 1 .. 64")
    _channel_tensor(d_values, None, torch.float64, "d_values")
    n_rows, n_ch = int(d_values.shape[0]), int(d_values.shape[1])
    device = d_values.device
    if matrix is None and factor is None:
        raise ValueError("correct_channels: neither a matrix nor a factor")
    if matrix is not None:
        if not isinstance(matrix, torch.Tensor):
            matrix = _upload(matrix, np.float64, device)
        _channel_tensor(matrix, (n_ch, n_ch), torch.float64, "matrix")
    if factor is not None:
        if not isinstance(factor, torch.Tensor):
            factor = _upload(factor, np.float64, device)
        _channel_tensor(factor, (n_ch,), torch.float64, "factor")
    if out is None:
        with torch.cuda.device(device):
            out = torch.empty((n_rows, n_ch), dtype=torch.float64, device=device)
    _channel_tensor(out, (n_rows, n_ch), torch.float64, "out")
    rc = scorer._lib.pya_channel_correct(scorer._h, d_values.data_ptr() if n_rows else None, n_rows, n_ch,
                                         None if matrix is None else matrix.data_ptr(), None if factor is None else factor.data_ptr(),
                                         torch.cuda.current_stream(device).cuda_stream, out.data_ptr() if n_rows else None)
    if rc:
        scorer._raise(rc)
    return out


def channel_sums(scorer, d_values, select=None, scale_log2=10, out=None):
    """SUMS of the channel correction over a device matrix (``pya_channel_sums``): ``d_values`` as ``correct_channels`` takes
    it, ``select`` a ``torch.uint8`` device tensor ``[n_rows]`` (0: the row is left out) or a host array of booleans or None for
    all rows.  ``out``: a contiguous ``torch.uint8`` device tensor ``[n_channels, 16]``, one ``pya_site_quant`` per channel, to
    ADD into; None: a new zeroed one.  Returns it (``channel_sum_records`` reads a host copy).  One launch on torch's current
    stream; nothing waits on the host.  ``pyascore_amd.rollup.channel_sums`` gives the same bytes."""
    import torch
    if not isinstance(scorer, PyAscore):
        raise TypeError("scorer must be a pyascore_amd.PyAscore")
    if d_values.dim() != 2 or not 1 <= d_values.shape[1] <= 64:
        raise ValueError("d_values must be a float64 device tensor of shape (n_rows, n_channels), n_channels in 1 .. 64")
    _channel_tensor(d_values, None, torch.float64, "d_values")
    n_rows, n_ch = int(d_values.shape[0]), int(d_values.shape[1])
    device = d_values.device
    if select is not None:
        if not isinstance(select, torch.Tensor):
            select = _upload(np.asarray(select) != 0, np.uint8, device)
        _channel_tensor(select, (n_rows,), torch.uint8, "select")
    if out is None:
        with torch.cuda.device(device):
            out = torch.zeros((n_ch, 16), dtype=torch.uint8, device=device)
    _channel_tensor(out, (n_ch, 16), torch.uint8, "out")
    rc = scorer._lib.pya_channel_sums(scorer._h, d_values.data_ptr() if n_rows else None, n_rows, n_ch,
                                      None if select is None or not n_rows else select.data_ptr(), int(scale_log2),
                                      torch.cuda.current_stream(device).cuda_stream, out.data_ptr())
    if rc:
        scorer._raise(rc)
    return out


def channel_factors(scorer, d_cell, out=None):
    """FACTORS of the channel correction (``pya_channel_factors``): ``d_cell`` the tensor of ``channel_sums`` (uint8
    ``[n_channels, 16]``); returns a ``torch.float64`` device tensor ``[n_channels]``, ``out`` when given.  One launch of one
    wavefront on torch's current stream; nothing waits on the host, so sums, factors and the second ``correct_channels`` chain
    without a host read.  ``pyascore_amd.rollup.channel_factors`` gives the same bytes."""
    import torch
    if not isinstance(scorer, PyAscore):
        raise TypeError("scorer must be a pyascore_amd.PyAscore")
    if d_cell.dim() != 2 or not 1 <= d_cell.shape[0] <= 64:
        raise ValueError("d_cell must be a uint8 device tensor of shape (n_channels, 16), n_channels in 1 .. 64")
    n_ch = int(d_cell.shape[0])
    _channel_tensor(d_cell, (n_ch, 16), torch.uint8, "d_cell")
    device = d_cell.device
    if out is None:
        with torch.cuda.device(device):
            out = torch.empty(n_ch, dtype=torch.float64, device=device)
    _channel_tensor(out, (n_ch,), torch.float64, "out")
    rc = scorer._lib.pya_channel_factors(scorer._h, d_cell.data_ptr(), n_ch, torch.cuda.current_stream(device).cuda_stream, out.data_ptr())
    if rc:
        scorer._raise(rc)
    return out


def channel_sum_records(raw):
    """A host copy of the tensor of ``channel_sums`` (``.cpu().numpy()``, uint8 ``[n_channels, 16]``) as the structured array
    ``pyascore_amd.rollup.channel_sums`` returns (``SITE_QUANT_DTYPE[n_channels]``); a view, no copy."""
    from .rollup import SITE_QUANT_DTYPE
    cell = np.ascontiguousarray(raw, np.uint8)
    if cell.ndim != 2 or cell.shape[1] != SITE_QUANT_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n_channels, 16)")
    return cell.view(SITE_QUANT_DTYPE).reshape(cell.shape[0])


def site_quant_records(raw):
    """Host copies of the table of ``DevicePlan.site_quant`` (``.cpu().numpy()`` of the pair: uint8 ``[n_slots, 8]`` and
    ``[n_slots, n_channels, 16]``) as the structured arrays ``PyAscore.score_batch(..., quant=...)`` returns in ``quant_head``
    and ``quant``; views, no copy."""
    from .rollup import SITE_QUANT_DTYPE, SITE_QUANT_HEAD_DTYPE
    head, cell = (np.ascontiguousarray(a, np.uint8) for a in raw)
    if head.ndim != 2 or head.shape[1] != SITE_QUANT_HEAD_DTYPE.itemsize or cell.ndim != 3 or cell.shape[2] != SITE_QUANT_DTYPE.itemsize \
            or cell.shape[0] != head.shape[0]:
        raise ValueError("expected uint8 arrays of shapes (n_slots, 8) and (n_slots, n_channels, 16)")
    return head.view(SITE_QUANT_HEAD_DTYPE).reshape(head.shape[0]), cell.view(SITE_QUANT_DTYPE).reshape(cell.shape[0], cell.shape[1])


def marker_records(raw):
    """A host copy of the first tensor of ``markers`` (``.cpu().numpy()``, uint8 ``[n_spectra, n_targets, 24]``) as the
    structured array ``PyAscore.score_batch(..., markers=...)`` returns in ``markers``; a view, no copy."""
    from .rollup import MARKER_DTYPE
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 3 or a.shape[2] != MARKER_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n_spectra, n_targets, %d)" % MARKER_DTYPE.itemsize)
    return a.view(MARKER_DTYPE).reshape(a.shape[0], a.shape[1])


def purity_records(raw):
    """A host copy of the tensor of ``purity`` (``.cpu().numpy()``, uint8 ``[n_query, 48]``) as the structured array
    ``PyAscore.score_batch(..., purity=...)`` returns in ``purity``; a view, no copy."""
    from .rollup import PURITY_DTYPE
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != PURITY_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % PURITY_DTYPE.itemsize)
    return a.view(PURITY_DTYPE).reshape(a.shape[0])


def xic_survey_check(scorer, d_ms1_mz, d_ms1_intensity, ms1_peak_off, out=None):
    """``scan_ok`` of the XIC stage over survey spectra that live on the device (``pya_xic_survey_check``): a ``uint8`` tensor
    ``[n_survey]``, 1 where the scan's m/z ascend.  The spectra as ``purity`` takes them; only the m/z are read.  ``out``: such a
    tensor to write into, new when None.  Run once per survey set: it serves every later ``xic`` call.  One launch on torch's
    current stream; nothing waits on the host.  ``pyascore_amd.rollup.survey_ascending`` gives the same bytes."""
    import torch
    _, device, peak_off, n_survey = _transform_inputs(scorer, lambda p: None, None, d_ms1_mz, d_ms1_intensity, ms1_peak_off)
    if out is None:
        with torch.cuda.device(device):
            out = torch.empty(n_survey, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n_survey,) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous uint8 device tensor of shape (%d,)" % n_survey)
    t_in = _lib.TypedSpectra(d_ms1_mz.data_ptr(), d_ms1_intensity.data_ptr(), _lib.spectrum_type(d_ms1_mz.dtype),
                             _lib.spectrum_type(d_ms1_intensity.dtype))
    rc = scorer._lib.pya_xic_survey_check(scorer._h, C.byref(t_in), peak_off.data_ptr(), n_survey, d_ms1_mz.numel(),
                                          torch.cuda.current_stream(device).cuda_stream, out.data_ptr() if n_survey else None)
    if rc:
        scorer._raise(rc)
    return out


def xic(scorer, d_ms1_mz, d_ms1_intensity, ms1_peak_off, d_rt, d_scan_ok, d_seed, d_scan_lo, d_scan_hi, d_prec_mz, d_prec_z, params, out=None):
    """The precursor XIC over survey spectra that live on the device (``pya_xic_spectra``; the rule is ``pya_xic_params``'s in
    include/pyascore_hip.h): the survey spectra as ``purity`` takes them; ``d_rt`` (float64 ``[n_survey]``, seconds) and
    ``d_scan_ok`` (uint8 ``[n_survey]``, of ``xic_survey_check``); ``d_seed`` / ``d_scan_lo`` / ``d_scan_hi`` (int64),
    ``d_prec_mz`` (float64), ``d_prec_z`` (int32) one entry per query -- device tensors or host arrays (a host array is
    uploaded); ``params`` of ``pyascore_amd.rollup.xic_params``.  ``out``: a contiguous ``uint8`` device tensor ``[n_query, 64]``
    to write into, new when None.  Returns ``(d_xic, d_over)``: the records (``xic_records`` reads a host copy; ``xic_values``
    makes the column the quant stages take) and an ``int32`` tensor of two words (the queries whose window is out of range, and
    0xffffffff minus the first of them).  READ-ONLY; one launch on torch's current stream; nothing waits on the host.
    ``pyascore_amd.rollup.xic`` gives the same bytes."""
    import torch
    from .rollup import XIC_DTYPE, xic_c_params
    c_params, device, peak_off, n_survey = _transform_inputs(scorer, xic_c_params, params, d_ms1_mz, d_ms1_intensity, ms1_peak_off)
    per_scan = []
    for t, np_dtype, dtype in ((d_rt, np.float64, torch.float64), (d_scan_ok, np.uint8, torch.uint8)):
        if not isinstance(t, torch.Tensor):
            t = _upload(t, np_dtype, device)
        if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda or t.numel() != n_survey:
            raise ValueError("d_rt (float64) and d_scan_ok (uint8) are contiguous device tensors with one entry per survey spectrum")
        per_scan.append(t)
    per_query = []
    for t, np_dtype, dtype in ((d_seed, np.int64, torch.int64), (d_scan_lo, np.int64, torch.int64), (d_scan_hi, np.int64, torch.int64),
                               (d_prec_mz, np.float64, torch.float64), (d_prec_z, np.int32, torch.int32)):
        if not isinstance(t, torch.Tensor):
            t = _upload(t, np_dtype, device)
        if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda or (per_query and t.numel() != per_query[0].numel()):
            raise ValueError("d_seed, d_scan_lo, d_scan_hi (int64), d_prec_mz (float64) and d_prec_z (int32) are contiguous device tensors "
                             "with one entry per query")
        per_query.append(t)
    n_query = per_query[0].numel()
    shape = (n_query, XIC_DTYPE.itemsize)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=device)
        over = torch.zeros(2, dtype=torch.int32, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous uint8 device tensor of shape %r" % (shape,))
    t_in = _lib.TypedSpectra(d_ms1_mz.data_ptr(), d_ms1_intensity.data_ptr(), _lib.spectrum_type(d_ms1_mz.dtype),
                             _lib.spectrum_type(d_ms1_intensity.dtype))
    rc = scorer._lib.pya_xic_spectra(scorer._h, C.byref(t_in), peak_off.data_ptr(), n_survey, d_ms1_mz.numel(),
                                     *(t.data_ptr() if n_survey else None for t in per_scan),
                                     *(t.data_ptr() if n_query else None for t in per_query), n_query, C.byref(c_params),
                                     torch.cuda.current_stream(device).cuda_stream, out.data_ptr() if n_query else None, over.data_ptr())
    if rc:
        scorer._raise(rc)
    # (the caching allocator keeps uploaded arrays for this stream until later work on the stream is done with them)
    return out, over


def xic_values(scorer, d_xic, which="area", out=None):
    """One column of the records of ``xic`` (uint8 ``[n, 64]``) as the one-channel matrix ``DevicePlan.site_quant`` and
    ``peptidoform_quant`` take (``pya_xic_values``): a ``torch.float64`` device tensor ``[n, 1]``, ``which`` 0 .. 3 or 'area',
    'apex', 'seed', 'sum'; NaN where the record is not SEEN or the value is not > 0.  ``out``: such a tensor to write into, new
    when None.  One launch on torch's current stream; nothing waits on the host.  ``pyascore_amd.rollup.xic_values`` gives the
    same bytes."""
    import torch
    from .rollup import XIC_DTYPE
    if not isinstance(scorer, PyAscore):
        raise TypeError("scorer must be a pyascore_amd.PyAscore")
    names = {"area": 0, "apex": 1, "seed": 2, "sum": 3}
    which = names.get(which, which) if isinstance(which, str) else which
    if isinstance(which, (bool, str)) or not isinstance(which, (int, np.integer)) or not 0 <= int(which) <= 3:
        raise ValueError("xic_values: which is 0 .. 3 or one of 'area', 'apex', 'seed', 'sum'")
    if d_xic.dim() != 2 or d_xic.shape[1] != XIC_DTYPE.itemsize:
        raise ValueError("d_xic must be a contiguous uint8 device tensor of shape (n, %d)" % XIC_DTYPE.itemsize)
    _channel_tensor(d_xic, None, torch.uint8, "d_xic")
    n, device = int(d_xic.shape[0]), d_xic.device
    if out is None:
        with torch.cuda.device(device):
            out = torch.empty((n, 1), dtype=torch.float64, device=device)
    _channel_tensor(out, (n, 1), torch.float64, "out")
    rc = scorer._lib.pya_xic_values(scorer._h, d_xic.data_ptr() if n else None, n, int(which), torch.cuda.current_stream(device).cuda_stream,
                                    out.data_ptr() if n else None)
    if rc:
        scorer._raise(rc)
    return out


def xic_records(raw):
    """A host copy of the tensor of ``xic`` (``.cpu().numpy()``, uint8 ``[n_query, 64]``) as the structured array
    ``PyAscore.precursor_xic`` returns; a view, no copy."""
    from .rollup import XIC_DTYPE
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != XIC_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % XIC_DTYPE.itemsize)
    return a.view(XIC_DTYPE).reshape(a.shape[0])


def marker_spectrum_records(raw):
    """A host copy of the second tensor of ``markers`` (``.cpu().numpy()``, uint8 ``[n_spectra, 32]``) as the structured
    array ``PyAscore.score_batch(..., markers=...)`` returns in ``marker_spectra``; a view, no copy."""
    from .rollup import MARKER_SPECTRUM_DTYPE
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != MARKER_SPECTRUM_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % MARKER_SPECTRUM_DTYPE.itemsize)
    return a.view(MARKER_SPECTRUM_DTYPE).reshape(a.shape[0])


def evidence_rows(raw):
    """A host copy of ``DevicePlan.evidence()`` (``.cpu().numpy()``, uint8 ``[n_psm, max_k, 16]``) as the structured
    array ``[n_psm, max_k]`` that ``PyAscore.score_batch(..., evidence=True)`` returns; a view, no copy."""
    a = np.ascontiguousarray(raw, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != EVIDENCE_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n_psm, max_k, %d)" % EVIDENCE_DTYPE.itemsize)
    return a.view(EVIDENCE_DTYPE).reshape(a.shape[0], a.shape[1])


def unpack_summary(packed, max_k):
    """Inverse of DevicePlan.packed_summary on a host int32 array -> dict of numpy arrays."""
    p = np.ascontiguousarray(packed, dtype=np.int32)
    k = max_k
    return dict(
        best_score=p[:, 0].copy().view(np.float32),
        n_sig=p[:, 1].copy(),
        best_sig=np.ascontiguousarray(p[:, 2:4]).view(np.uint64).reshape(-1),
        ascores=np.ascontiguousarray(p[:, 4:4 + k]).view(np.float32),
        alt_mask=np.ascontiguousarray(p[:, 4 + k:4 + 3 * k]).view(np.uint64).reshape(-1, k),
    )


def ion_records(raw):
    """A host copy of the records of ``DevicePlan.ions()`` (``.cpu().numpy()``, uint8 ``[total, 16]``) as the structured
    array ``PyAscore.score_batch(..., ions=True)`` returns; a view, no copy."""
    a = np.ascontiguousarray(raw)
    if a.ndim != 2 or a.shape[1] != ION_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (total, %d)" % ION_DTYPE.itemsize)
    return a.view(ION_DTYPE).reshape(a.shape[0])


def site_records(raw):
    """A host copy of the records of ``DevicePlan.sites()`` (``.cpu().numpy()``, uint8 ``[n, 32]``) as the structured array
    ``PyAscore.score_batch(..., sites=True)`` returns; a view, no copy."""
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != SITE_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % SITE_DTYPE.itemsize)
    return a.view(SITE_DTYPE).reshape(a.shape[0])


def psm_prob_records(raw):
    """A host copy of the PSM records of ``DevicePlan.probs()`` (``.cpu().numpy()``, uint8 ``[n, 16]``) as the structured
    array ``PyAscore.score_batch(..., probs=True)`` returns in ``psm_probs``; a view, no copy."""
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != PSM_PROB_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % PSM_PROB_DTYPE.itemsize)
    return a.view(PSM_PROB_DTYPE).reshape(a.shape[0])


def ranked_records(raw):
    """A host copy of the records of ``DevicePlan.ranked()`` (``.cpu().numpy()``, uint8 ``[n, K, 16]``) as the structured
    array ``PyAscore.score_batch(..., ranked=K)`` returns in ``ranked``, shape ``[n, K]``; a view, no copy."""
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 3 or a.shape[2] != RANKED_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, K, %d)" % RANKED_DTYPE.itemsize)
    return a.view(RANKED_DTYPE).reshape(a.shape[0], a.shape[1])


def rollup_records(raw):
    """A host copy of a roll-up table (``.cpu().numpy()``, uint8 ``[n_slots, 32]``) as the structured array
    ``PyAscore.score_batch(..., rollup=...)`` returns in ``rollup``; a view, no copy."""
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != ROLLUP_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % ROLLUP_DTYPE.itemsize)
    return a.view(ROLLUP_DTYPE).reshape(a.shape[0])


def coverage_records(raw):
    """A host copy of the records of ``DevicePlan.coverage()`` (``.cpu().numpy()``, uint8 ``[n, 64]``) as the structured
    array ``PyAscore.score_batch(..., coverage=True)`` returns; a view, no copy."""
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != COVERAGE_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % COVERAGE_DTYPE.itemsize)
    return a.view(COVERAGE_DTYPE).reshape(a.shape[0])


def mz_profile_records(raw):
    """A host copy of a mass-error profile table (``.cpu().numpy()``, uint8 ``[n_slots, 4128]``) as the structured array
    ``PyAscore.score_batch(..., mz_profile=...)`` returns in ``mz_profile``; a view, no copy."""
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != MZ_PROFILE_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % MZ_PROFILE_DTYPE.itemsize)
    return a.view(MZ_PROFILE_DTYPE).reshape(a.shape[0])


def mz_calibration_records(raw):
    """A host copy of the calibration of ``DevicePlan.fit_mz_calibration()`` (``.cpu().numpy()``, uint8 ``[n_slots, 128]``) as
    the structured array ``PyAscore.fit_mz_calibration`` returns (``pyascore_amd.rollup.MZ_CALIBRATION_DTYPE``); a view, no
    copy."""
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != MZ_CALIBRATION_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % MZ_CALIBRATION_DTYPE.itemsize)
    return a.view(MZ_CALIBRATION_DTYPE).reshape(a.shape[0])


def peptidoform_records(raw):
    """A host copy of the records of ``DevicePlan.peptidoforms()`` / ``peptidoform_reduce()`` (``[:n].cpu().numpy()``, uint8
    ``[n, 48]``) as the structured array ``PyAscore.score_batch(..., peptidoforms=...)`` returns; a view, no copy."""
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != PEPTIDOFORM_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % PEPTIDOFORM_DTYPE.itemsize)
    return a.view(PEPTIDOFORM_DTYPE).reshape(a.shape[0])


def flr_records(raw):
    """A host copy of the records of ``DevicePlan.rollup_flr()`` (``.cpu().numpy()``, uint8 ``[n_slots, 32]``) as the
    structured array ``PyAscore.rollup_flr`` returns; a view, no copy."""
    a = np.ascontiguousarray(raw, np.uint8)
    if a.ndim != 2 or a.shape[1] != FLR_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n, %d)" % FLR_DTYPE.itemsize)
    return a.view(FLR_DTYPE).reshape(a.shape[0])


def named_records(raw):
    """A host copy of the records of ``DevicePlan.named()`` (``.cpu().numpy()``, uint8 ``[n_q, 32]``) as the structured
    array ``PyAscore.score_batch(..., named=...)`` returns; a view, no copy."""
    a = np.ascontiguousarray(raw)
    if a.ndim != 2 or a.shape[1] != NAMED_DTYPE.itemsize:
        raise ValueError("expected a uint8 array of shape (n_q, %d)" % NAMED_DTYPE.itemsize)
    return a.view(NAMED_DTYPE).reshape(a.shape[0])
