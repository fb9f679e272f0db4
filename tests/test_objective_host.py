"""CPU: the host decisions of the one-pass objective's call -- ops._MappedHints.plan / counted: launch sizes, counters, a pending record-slot
overflow, compact or per-pixel records, the count-only call -- and fit.step_path, which of its four forms a fit step runs.
Neither needs a device: the hint record is driven by writing its host words the way k_objective_finish does."""
import itertools

import pytest
import torch

import fpc_diffrend_amd.ops as dr
from fpc_diffrend_amd import _lib, fit

BIN2 = _lib.OCC_BIN * _lib.OCC_BIN
N_PIX = 123457      # (B * H * W of the call: what a by-pixel record pool holds)


def device_writes(h, seq, counters, overflow=False, slots_valid=1):
    """k_objective_finish (include/fpcdr.h counts_out): [6] = seq, [deferred bins, slot demand, live bins, occupied bins], [5] += overflow,
    [7], then [4] = seq."""
    h.host[6] = seq
    h.host[:4] = torch.tensor(counters, dtype=torch.int32)
    if overflow:
        h.host[5] += 1
    h.host[7] = slots_valid
    h.host[4] = seq


def plan(h, nbins, capturing=False, skip_out=False, record_slots=None):
    return dr._MappedHints.plan(h, nbins, capturing, skip_out, record_slots, N_PIX)


def margin(n):
    return n + max(256, n // 8)


def test_no_hint_record_runs_unhinted_unreported_and_by_pixel_unless_told():
    for capturing, skip_out in itertools.product((False, True), repeat=2):
        p = plan(None, 50000, capturing, skip_out)
        assert p == ((0, 0, 0), None, False, 0, N_PIX) and p.n_records == N_PIX
        p = plan(None, 50000, capturing, skip_out, record_slots=7)
        assert (p.caps, p.seq, p.count, p.slots, p.n_records) == ((0, 0, 0), None, False, 7, 7 * BIN2)
        assert plan(None, 50000, capturing, skip_out, record_slots=0).n_records == N_PIX


def test_plan_table_of_a_hint_record(monkeypatch):
    h = dr._MappedHints()
    small, large = dr.SMALL_BATCH_BINS, dr.SMALL_BATCH_BINS + 1
    # a fresh record, small batch: caps 0, counters handed over under a fresh number, records by pixel, nothing counted first
    p = plan(h, small)
    assert (p.caps, p.seq, p.count, p.slots, p.n_records) == ((0, 0, 0), 1, False, 0, N_PIX) and h.seq == 1
    device_writes(h, p.seq, [40, 500, 8000, 7000])
    caps = (margin(8000), margin(7000), margin(40))
    # ... its counters have landed: a small batch still runs at its full size, a batch one bin larger takes the caps
    p = plan(h, small)
    assert p.caps == (0, 0, 0) and p.seq == 2 and h.caps == caps
    p = plan(h, large)
    assert p.caps == caps and p.seq == 3
    # compact by itself beyond SMALL_BATCH_BINS: the slots the last call seen asks for; no count, its demand is known
    assert h.sil_bins == 500 and h.slots == 500 + max(dr.RECORD_SLOT_MARGIN, 250)
    assert (p.count, p.slots, p.n_records) == (False, h.slots, h.slots * BIN2)
    assert plan(h, small).slots == 0
    # record_slots wins, 0 included, whatever the record says
    for nbins, given in itertools.product((small, large), (0, 3)):
        p = plan(h, nbins, record_slots=given)
        assert (p.count, p.slots, p.n_records) == (False, given, given * BIN2 if given else N_PIX)
    # COMPACT_RECORDS off: by pixel at any size
    monkeypatch.setattr(dr, "COMPACT_RECORDS", False)
    p = plan(h, large)
    assert (p.caps, p.count, p.slots, p.n_records) == (caps, False, 0, N_PIX)
    monkeypatch.setattr(dr, "COMPACT_RECORDS", True)
    # under capture: sized launches, but nothing reported (no sequence number drawn), records by pixel
    seq = h.seq
    p = plan(h, large, capturing=True)
    assert (p.caps, p.seq, p.count, p.slots, p.n_records) == (caps, None, False, 0, N_PIX) and h.seq == seq
    assert plan(h, large, capturing=True, record_slots=5).slots == 5
    # a frozen record keeps its caps at any size, and never counts: slots are max(slots, 1)
    f = dr._MappedHints()
    f.frozen, f.caps = True, (3, 2, 1)
    assert plan(f, 1).caps == (3, 2, 1) and plan(f, large).caps == (3, 2, 1)
    p = plan(f, large)
    assert f.sil_bins < 0 and (p.count, p.slots, p.n_records) == (False, 1, BIN2)
    f.slots = 9
    assert plan(f, large).slots == 9 and plan(f, small).slots == 0


def test_count_only_call_and_slot_arithmetic(monkeypatch):
    monkeypatch.setattr(dr, "SMALL_BATCH_BINS", 0)
    monkeypatch.setattr(dr, "RECORD_SLOT_MARGIN", 1)
    h = dr._MappedHints()
    # first call on a shape: nothing seen yet -- count first, with the counters handed over
    p = plan(h, 4)
    assert (p.caps, p.seq, p.count) == ((0, 0, 0), 1, True)
    # the counting call reported nothing (the caller waited for the stream, and still no counters)
    with pytest.raises(RuntimeError, match="the counting call reported nothing"):
        h.counted(p)
    assert plan(h, 4).count is True
    # a count lands: caps re-polled, a FRESH number, slots = sil + max(RECORD_SLOT_MARGIN, sil // 2), nothing more to count
    for sil in (0, 1, 2, 7, 501):
        h = dr._MappedHints()
        p = plan(h, 4)
        device_writes(h, p.seq, [2, sil, 4, 3])
        q = h.counted(p)
        want = max(sil + max(dr.RECORD_SLOT_MARGIN, sil // 2), 1)
        assert want == max(sil + max(1, sil // 2), 1)
        assert (q.caps, q.seq, q.count, q.slots, q.n_records) == ((margin(4), margin(3), margin(2)), p.seq + 1, False, want, want * BIN2)
        nxt = plan(h, 4)
        assert (nxt.caps, nxt.seq, nxt.count, nxt.slots) == (q.caps, q.seq + 1, False, want)
    # record_slots given, capture, COMPACT_RECORDS off: no count even though nothing has been seen
    h = dr._MappedHints()
    assert plan(h, 4, record_slots=2).count is False and plan(h, 4, capturing=True).count is False
    monkeypatch.setattr(dr, "COMPACT_RECORDS", False)
    assert plan(h, 4).count is False
    # the default margin
    monkeypatch.undo()
    h = dr._MappedHints()
    device_writes(h, h.next_seq(), [1, 100, 9, 9])
    assert plan(h, dr.SMALL_BATCH_BINS + 1).slots == 100 + 1024 == 100 + max(dr.RECORD_SLOT_MARGIN, 50)


def test_a_pending_overflow_is_consumed_once_raised_or_counted_as_skipped(monkeypatch):
    monkeypatch.setattr(dr, "SMALL_BATCH_BINS", 0)
    monkeypatch.setattr(dr, "RECORD_SLOT_MARGIN", 1)

    def overflowed_record():
        h = dr._MappedHints()
        device_writes(h, h.next_seq(), [2, 10, 4, 3])
        assert plan(h, 4).slots == 15 and h.overflowed is None
        device_writes(h, h.seq, [2, 40, 4, 3], overflow=True)      # that call ran out: it kept counting beyond its pool
        return h

    # with skip_out: the caller had the device flag -- no raise, a skipped call counted, the demand it counted sizes this call
    h = overflowed_record()
    p = plan(h, 4, skip_out=True)
    assert h.overflowed is None and h.skipped_calls == 1 and h.overflow_count == 1
    assert (p.count, p.slots, p.seq) == (False, 40 + 20, 3)
    assert plan(h, 4, skip_out=True).slots == 60 and h.skipped_calls == 1      # (consumed once)
    # without: the existing RuntimeError, and a re-count in front of the next call
    h = overflowed_record()
    with pytest.raises(RuntimeError, match=r"pixel_objective: a call on this batch shape \(sequence number <= 2\) ran out of record slots \(the "
                       r"take's silhouette grew by more than half within one step\); its value was NaN and its gradients incomplete -- "
                       r"repeat the step, or pass skip_out= and skip the update as Fitter does$"):
        plan(h, 4)
    assert h.overflowed is None and h.sil_bins == -1 and h.skipped_calls == 0 and h.seq == 3
    p = plan(h, 4)
    assert p.count is True and p.seq == 4
    # a caller that names its slots learns it the same way
    h = overflowed_record()
    with pytest.raises(RuntimeError, match="ran out of record slots"):
        plan(h, 4, record_slots=0)
    # a captured call leaves it pending, with or without skip_out; the next eager call takes it
    h = overflowed_record()
    for skip_out in (False, True):
        p = plan(h, 4, capturing=True, skip_out=skip_out)
        assert h.overflowed == 2 and h.skipped_calls == 0 and (p.seq, p.slots) == (None, 0)
    plan(h, 4, skip_out=True)
    assert h.overflowed is None and h.skipped_calls == 1
    # a frozen record sees it too
    h = overflowed_record()
    h.frozen = True
    with pytest.raises(RuntimeError, match="ran out of record slots"):
        plan(h, 4)


FLAGS = ("fused_objective", "fused_render", "fused_loss", "one_pass", "sparse_objective")


def test_step_path_names_the_form_the_step_ran_before_it_was_asked_once():
    from fpc_diffrend_amd.fit import weighted_one_pass_term

    def parent_form(cfg, term, mip, C):
        """Fitter.loss_and_backward's expressions in front of step_path, and the branch they led to."""
        one_shot = (cfg.fused_objective and cfg.fused_render and cfg.fused_loss and C in (1, 3, 4) and cfg.shading == 'texture'
                    and (not mip or cfg.sparse_objective))
        weighted_shot = bool(cfg.weighted_one_pass and term is not None and term[0] == 'robust' and cfg.fused_objective and cfg.fused_render
                             and cfg.fused_loss and cfg.one_pass and cfg.sparse_objective and cfg.shading == 'texture' and C in (1, 3, 4)
                             and not mip)
        one_shot = one_shot and (term is None or weighted_shot)
        if one_shot:      # (ops.pixel_objective(one_pass=cfg.one_pass, sparse=cfg.sparse_objective) picks its form by these two)
            return ('one_pass' if (cfg.one_pass and cfg.sparse_objective) else 'two_call'), weighted_shot
        return ('operators' if cfg.fused_loss else 'torch'), False

    cfg = fit.FitConfig()
    terms = (None, ('blur', dr.gaussian_taps(15, 3.0)), ('robust', 'charbonnier', 10.0))
    seen = set()
    for flags in itertools.product((False, True), repeat=len(FLAGS)):
        for name, on in zip(FLAGS, flags):
            setattr(cfg, name, on)
        for shading, C, mip, term, w1p in itertools.product(('texture', 'vertex'), (1, 2, 3, 4), (False, True), terms, (False, True)):
            cfg.shading, cfg.weighted_one_pass = shading, w1p
            want = parent_form(cfg, term, mip, C)
            got = fit.step_path(cfg, term, mip, C)
            assert got == want and type(got[1]) is bool, (flags, shading, C, mip, term, w1p, got, want)
            assert weighted_one_pass_term(cfg, term, mip, C) is want[1]
            seen.add(got)
    assert seen == {('one_pass', False), ('one_pass', True), ('two_call', False), ('operators', False), ('torch', False)}
    # the defaults: the plain one-pass step; a windowed term, vertex shading or two channels: the operators
    cfg = fit.FitConfig()
    assert fit.step_path(cfg, None, False) == fit.step_path(cfg, None, True, 3) == ('one_pass', False)
    assert fit.step_path(cfg, terms[1], False) == fit.step_path(cfg, None, False, 2) == ('operators', False)
    assert fit.step_path(fit.FitConfig(shading='vertex'), None, False) == ('operators', False)
    assert fit.step_path(fit.FitConfig(one_pass=False), None, True) == ('two_call', False)
    assert fit.step_path(fit.FitConfig(sparse_objective=False), None, True) == ('operators', False)      # (mip needs the sparse form)
    assert fit.step_path(fit.FitConfig(fused_loss=False), None, False) == ('torch', False)
