"""Range audit of the tensors the detector STORES between layers (csrc/range_probe.hip).

The fp16-pair arithmetic ('f16x2') is only as safe as the power-of-two pre-scale `select_math` picks: the split of csrc/hgemm.h clamps
to +-65504 silently.  While a ``RangeAudit`` is recording, every convolution of the sparse backbone, the BEV backbone and the head's
dense stage probes its output once per pass, after the last launch that writes it, into a device record of its own (peak, saturated,
nonfinite, elements).  Nothing is synchronised or allocated by a probe after the first eager pass, so an audited pass captures into a
graph like any other; ``report()`` makes the one host copy.

Out of the audit: values that never reach memory - the hidden activations of the regression branches evaluated at the top-K cells
(csrc/head_cand.hip keeps them in registers), accumulators, the voxel features (stored unscaled).
"""
import contextlib
import math

import torch

from . import ops
from .lib import DetZeroHipError

_ACTIVE = [None]         # the recording audit (module-level hook, in the manner of det_modules._WORKSPACE)
F16_MAX = 65504.0


def active():
    """The audit that is recording, or None: the one test a layer makes on the host."""
    return _ACTIVE[0]


class RangeAudit:
    def __init__(self, capacity=256):
        self.capacity = int(capacity)
        self.table = None
        self.records = {}            # name -> {'slot', 'stage', 'exp', 'storage'} in first-probe order

    @contextlib.contextmanager
    def recording(self):
        prev = _ACTIVE[0]
        _ACTIVE[0] = self
        try:
            yield self
        finally:
            _ACTIVE[0] = prev

    def _slot(self, name, t, stage, exp, storage):
        rec = self.records.get(name)
        if rec is None:
            if torch.cuda.is_current_stream_capturing():
                raise DetZeroHipError('RangeAudit: tensor %r is first seen inside a graph capture - run one eager pass under the audit first '
                                      '(slots are assigned and the table allocated there)' % name)
            if self.table is None:
                self.table = ops.range_table(self.capacity, t.device)
            if len(self.records) >= self.capacity:
                raise DetZeroHipError('RangeAudit: more than %d tensors - construct it with a larger capacity' % self.capacity)
            rec = self.records[name] = {'slot': len(self.records)}
        # (the group, exponent and storage in force are those of the latest pass: set_math / set_prescale between passes change them)
        rec['stage'], rec['exp'], rec['storage'] = stage, int(exp), int(storage)
        return self.table[rec['slot']]

    def probe(self, name, t, *, math, stage, exp=0, rows=None, d_rows=None, c_off=0, c=None):
        """One probe of tensor `t` (ops.range_probe's arguments) into the record of `name`.  stage: the tensor's exponent group (one of
        centerpoint.PRESCALE_STAGES, None for an fp32 output), exp: the exponent in force (the tensor holds value * 2^exp)."""
        storage = ops.storage_math(math)
        ops.range_probe(t, self._slot(name, t, stage, exp, storage), math=storage, rows=rows, d_rows=d_rows, c_off=c_off, c=c)

    def reset(self):
        if self.table is not None:
            ops.range_reset(self.table)

    def report(self):
        """One host copy -> a list of dicts in first-probe order: name, stage, exp, storage ('f32' | 'f16x2' | 'bf16x2'), peak_stored,
        peak (= peak_stored * 2^-exp, the activation itself), saturated, nonfinite, elements, headroom_bits (fp16 pairs:
        log2(65504 / peak_stored); None otherwise)."""
        if self.table is None:
            return []
        raw = ops.range_read(self.table)
        names = {0: 'f32', 1: 'f16x2', 2: 'bf16x2'}
        out = []
        for name, rec in self.records.items():
            r = raw[rec['slot']]
            stored = float(r['peak'])
            out.append({'name': name, 'stage': rec['stage'], 'exp': rec['exp'], 'storage': names[rec['storage']], 'peak_stored': stored,
                        'peak': math.ldexp(stored, -rec['exp']), 'saturated': int(r['saturated']), 'nonfinite': int(r['nonfinite']),
                        'elements': int(r['elements']),
                        'headroom_bits': (math.log2(F16_MAX / stored) if stored > 0.0 else math.inf) if rec['storage'] == 1 else None})
        return out


def first_violation(report):
    """The first record of a report with a saturated or non-finite element, or None."""
    for r in report:
        if r['saturated'] > 0 or r['nonfinite'] > 0:
            return r
    return None


def describe(r):
    return ('%s: %d saturated, %d non-finite of %d elements (peak %.6g, stored peak %.6g at exponent %d, stage %s, %s storage)'
            % (r['name'], r['saturated'], r['nonfinite'], r['elements'], r['peak'], r['peak_stored'], r['exp'], r['stage'], r['storage']))
