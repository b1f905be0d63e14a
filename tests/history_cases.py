"""State model of the handles' HISTORY: what a `la_synth` / `la_disc` / `la_feat` / `la_latent_opt` handle did before a pass must not reach
the pass.  Shared by test_history_cases_cpu.py (coverage, determinism, plan proofs; no GPU) and test_hip_history.py (which runs every
history on a used handle and compares the probe, bit for bit, with a newly created handle).  No GPU, no ctypes and no torch here.

A HISTORY is a list of 3..6 operations followed by a PROBE.  Operations are tuples (name, argument, ...); the host-side state they leave
is restated by the `*Model` classes below (windows, precision, schedule, the kind of the last pass, its batch), which also say whether
an operation is valid where it stands and what a refused call returns.  The model proves reach only; no expected value comes from it.

    PAIRWISE[kind]   hand-written, so that every ordered pair (state class before the probe, state class of the probe) of the
                     tables `REQUIRED[kind]` occurs at least once: `reach(kind)` returns {axis: {(before, probe): [history names]}}
    RANDOM[kind]     8 histories drawn by `random_history` from random.Random(seed) with the seeds written below: the same operations,
                     the same length limit

History passes run on inputs scaled as `pass_scale` says: the latents (images, for the discriminator and the feature engine) by 2^3
and the gradients by 2^8 on the even passes of a history, both by 2^-6 on the odd ones, so that a stale operand scale, plane maximum or
partial is far from the probe's on either side.  The probe runs on the plain seeded inputs of the existing case tables.

Synthesis state classes (one value per axis):
    win    'whole' | 'row' | 'rowcol'          the window set on the handle
    prec   'f32' | 'bf16x3' | 'f16x2'
    sched  0 | 1                               la_synth_set_torgb_schedule
    last   'none' | 'bwd' | 'nbwd'             what followed the last forward pass: nothing, a backward, a noise backward
    brel   'larger' | 'equal' | 'smaller'      batch of the last forward pass against the probe's
Pairs required: every (before, probe) within win, prec and sched; every `last` and every `brel` value in front of the probe; and the two
crosses (win before, prec of the probe), (prec before, win of the probe).  Not the full product.
"""
import random

MODES = ('f32', 'bf16x3', 'f16x2')
LEN_MIN, LEN_MAX = 3, 6
MAX_BATCH = 4
WS_SCALE, G_SCALE, SMALL_SCALE = 2.0 ** 3, 2.0 ** 8, 2.0 ** -6
LA_OK, LA_ERR_ARG = 0, -1


def pass_scale(index):
    """(factor on the latents / images, factor on the gradients) of the index-th forward pass of a history"""
    return (WS_SCALE, G_SCALE) if index % 2 == 0 else (SMALL_SCALE, SMALL_SCALE)


class History:
    def __init__(self, name, case, ops, probe):
        self.name, self.case, self.ops, self.probe = name, case, [tuple(o) for o in ops], dict(probe)

    def __repr__(self):
        return f'History({self.name!r}, {self.case!r}, {self.ops!r}, {self.probe!r})'


# ---------------------------------------------------------------------------------------------------------------------------------
# synthesis engine

def window_of(R):
    return R // 4 + 1, 3 * R // 4 - 2          # synth_cases.window_of


# shapes: name -> (R, rows the case may window, column windows it may add).  `chain`: the two R = 64 tables of test_hip_image_chain.py
SYNTH_SHAPES = {
    'R16-imgc3-ch12-20-8': dict(R=16, rows=[], cols=[]),
    'synth-shrinking-batch': dict(R=16, rows=[], cols=[]),
    'chain:r64_f16x2_top_fuses': dict(R=64, rows=[], cols=[]),          # 32 channels everywhere: the top block fuses its ToRGB, the chain is deferred
    'chain:r64_f16x2': dict(R=64, rows=[], cols=[]),                    # 16 channels at 64^2: no fused block
    'R64-rgbfuse-imgc3': dict(R=64, rows=[window_of(64), (0, 16)], cols=[]),
    'R128-imgc3': dict(R=128, rows=[window_of(128), (0, 32)], cols=[(27, 101), (70, 122), window_of(128)]),
}
COLS_PLANNED_AWAY = (27, 101)          # its 32-column tiles are the whole row: la_synth.hip plans no column window (test_hip_col_window_up.py)
SYNTH_PROBE_B = 2


class SynthModel:
    """host-side state of a la_synth handle"""

    def __init__(self, prec='f32'):
        self.rows, self.cols, self.prec, self.sched = (0, 0), (0, 0), prec, 0
        self.last, self.lastB, self.fwd = 'none', None, None          # fwd: settings the last forward pass ran with
        self.passes = 0

    @property
    def win(self):
        return 'whole' if self.rows[1] == 0 else ('row' if self.cols[1] == 0 else 'rowcol')

    def state(self, probe_B):
        brel = None if self.lastB is None else ('larger' if self.lastB > probe_B else 'smaller' if self.lastB < probe_B else 'equal')
        return dict(win=self.win, prec=self.prec, sched=self.sched, last=self.last, brel=brel)

    def windowed_pass(self):
        """the last forward ran with a window set, or one is set now: what la_synth_backward_noise refuses noise gradients for"""
        return self.rows[1] > 0 or self.cols[1] > 0 or (self.fwd is not None and (self.fwd['rows'][1] > 0 or self.fwd['cols'][1] > 0))

    def valid(self, op):
        name = op[0]
        if name in ('backward', 'refused_noise', 'backward_noise'):
            if self.fwd is None:
                return False
            if name == 'backward_noise':
                return not self.windowed_pass()
            if name == 'refused_noise':          # (certain only while a window is set: a window of the forward pass alone refuses where it was planned)
                return self.rows[1] > 0
        if name == 'set_cols':
            return self.rows[1] > 0          # columns go on top of a row window
        return True

    def apply(self, op):
        """-> the status the call must return"""
        name = op[0]
        assert self.valid(op), (op, vars(self))
        if name == 'forward':
            self.fwd = dict(B=op[1], rows=self.rows, cols=self.cols, prec=self.prec, sched=self.sched, index=self.passes)
            self.passes += 1
            self.last, self.lastB = 'none', op[1]
        elif name == 'backward':
            self.last = 'bwd'
        elif name == 'backward_noise':
            self.last = 'nbwd'
        elif name == 'set_precision':
            self.prec = op[1]
        elif name == 'set_schedule':
            self.sched = op[1]
        elif name == 'set_rows':
            self.rows = tuple(op[1:3])
        elif name == 'set_cols':
            self.cols = tuple(op[1:3])
        elif name == 'clear_windows':
            self.rows = self.cols = (0, 0)
        elif name in ('refused_forward', 'refused_noise'):
            return LA_ERR_ARG
        else:
            raise ValueError(name)
        return LA_OK


def fwd(B, noise=1, wplus=True, out=True):
    """forward(B, noise_mode 0 none | 1 const | 2 explicit, ws_lstride w_dim (wplus) or 0, img_out given or NULL)"""
    return ('forward', B, noise, wplus, out)


def rows(lo, hi):
    return ('set_rows', lo, hi)


def cols(lo, hi):
    return ('set_cols', lo, hi)


def prec(mode):
    return ('set_precision', mode)


def sched(v):
    return ('set_schedule', v)


BWD, NBWD, CLEAR, REF_FWD, REF_NOISE = ('backward',), ('backward_noise',), ('clear_windows',), ('refused_forward',), ('refused_noise',)
W128, TOP128, W64, TOP64 = window_of(128), (0, 32), window_of(64), (0, 16)
WINS = ('whole', 'row', 'rowcol')


def sprobe(prec='f32', sched=0, rows=(0, 0), cols=(0, 0)):
    return dict(B=SYNTH_PROBE_B, prec=prec, sched=sched, rows=tuple(rows), cols=tuple(cols))


def probe_win(p):
    return 'whole' if p['rows'][1] == 0 else ('row' if p['cols'][1] == 0 else 'rowcol')


def _oa9():
    """R128-imgc3: the orthogonal array OA(9, 4, 3, 2) over (win before, prec before, win of the probe, prec of the probe) = (a, b, a + b,
    a + 2 b) mod 3 -- every pair of two of the four columns occurs once, which is the win pairs, the prec pairs and both crosses"""
    out = []
    setwin = {'whole': [], 'row': [rows(*W128)], 'rowcol': [rows(*W128), cols(70, 122)]}
    pwin = {'whole': dict(), 'row': dict(rows=W128), 'rowcol': dict(rows=W128, cols=(70, 122))}
    # the operations that follow the window and precision setters differ from history to history: 1..3 of them, batch 1..4
    tails = [[fwd(4), BWD], [fwd(3, 0, False), BWD, fwd(1)], [fwd(2), BWD], [fwd(4, 1, True, False)], [fwd(1), BWD], [fwd(3), BWD, REF_FWD],
             [fwd(2, 0), BWD], [fwd(4), BWD, fwd(2, 1, False)], [fwd(1, 1, True, False), BWD]]
    for a in range(3):
        for b in range(3):
            wb, pb, wp, pp = WINS[a], MODES[b], WINS[(a + b) % 3], MODES[(a + 2 * b) % 3]
            ops = [prec(pb)] + setwin[wb] + tails[3 * a + b]
            out.append(History(f'oa-{wb}-{pb}-to-{wp}-{pp}', 'R128-imgc3', ops, sprobe(pp, **pwin[wp])))
    return out


PAIRWISE = {}
PAIRWISE['synth'] = _oa9() + [
    # suspect 3 of the issue: window A -> whole frame with large values -> window B -> window A
    History('rows-A-whole-B-then-A', 'R128-imgc3', [prec('f16x2'), rows(*W128), fwd(2), CLEAR, fwd(4), rows(*TOP128)], sprobe('f16x2', rows=W128)),
    History('rows-B-pass-then-A', 'R128-imgc3', [prec('bf16x3'), rows(*TOP128), fwd(4), BWD, rows(*W128), fwd(3)], sprobe('bf16x3', rows=W128)),
    History('cols-right-edge-then-planned-away', 'R128-imgc3', [prec('f16x2'), rows(*W128), cols(70, 122), fwd(4), BWD], sprobe('f16x2', rows=W128, cols=COLS_PLANNED_AWAY)),
    History('cols-planned-away-then-right-edge', 'R128-imgc3', [prec('f16x2'), rows(*W128), cols(*COLS_PLANNED_AWAY), fwd(3), BWD], sprobe('f16x2', rows=W128, cols=(70, 122))),
    History('cols-window-of-then-top-rows', 'R128-imgc3', [prec('bf16x3'), rows(*W128), cols(*W128), fwd(2), BWD], sprobe('bf16x3', rows=TOP128)),
    # refused noise gradient while a window is set; a window changed between forward and backward
    History('refused-noise-in-window', 'R128-imgc3', [prec('f16x2'), rows(*W128), fwd(2), REF_NOISE, BWD], sprobe('f16x2')),
    History('window-set-after-forward', 'R128-imgc3', [prec('f16x2'), fwd(3), rows(*W128), BWD], sprobe('f16x2', rows=W128)),
    History('window-cleared-after-forward', 'R128-imgc3', [prec('bf16x3'), rows(*TOP128), fwd(2), CLEAR, BWD], sprobe('bf16x3')),
    # rows with the fused ToRGB block at 64^2
    History('r64-rows-then-whole', 'R64-rgbfuse-imgc3', [prec('f16x2'), rows(*W64), fwd(4), BWD], sprobe('f16x2')),
    History('r64-whole-then-rows', 'R64-rgbfuse-imgc3', [prec('f16x2'), fwd(4), BWD, fwd(1)], sprobe('f16x2', rows=W64)),
    History('r64-top-rows-then-rows', 'R64-rgbfuse-imgc3', [prec('bf16x3'), rows(*TOP64), fwd(3), BWD, REF_NOISE], sprobe('bf16x3', rows=W64)),
    History('r64-rows-then-top-rows', 'R64-rgbfuse-imgc3', [prec('bf16x3'), rows(*W64), fwd(2), CLEAR, fwd(4, 0)], sprobe('f16x2', rows=TOP64)),
    # the ToRGB schedule: all four pairs on each of the two tables (fused top block: deferred chain; no fused block)
    History('sched-0-to-0-fused', 'chain:r64_f16x2_top_fuses', [prec('f16x2'), fwd(4), BWD], sprobe('f16x2', 0)),
    History('sched-0-to-1-fused', 'chain:r64_f16x2_top_fuses', [prec('f16x2'), fwd(3), NBWD], sprobe('f16x2', 1)),
    History('sched-1-to-0-fused', 'chain:r64_f16x2_top_fuses', [prec('f16x2'), sched(1), fwd(4), BWD], sprobe('f16x2', 0)),
    History('sched-1-to-1-fused', 'chain:r64_f16x2_top_fuses', [prec('bf16x3'), sched(1), fwd(1), BWD], sprobe('bf16x3', 1)),
    History('sched-0-to-1-plain', 'chain:r64_f16x2', [prec('f16x2'), fwd(4), BWD], sprobe('f16x2', 1)),
    History('sched-1-to-0-plain', 'chain:r64_f16x2', [prec('f16x2'), sched(1), fwd(3), NBWD], sprobe('f16x2', 0)),
    History('sched-changed-after-forward', 'chain:r64_f16x2_top_fuses', [prec('f16x2'), fwd(2), sched(1), BWD], sprobe('f16x2', 1)),
    History('sched-1-f32-to-0', 'chain:r64_f16x2', [sched(1), fwd(4), BWD], sprobe('f32', 0)),
    # no windows: precision, the kind of the last pass, the batch, noise modes, ws_lstride, img_out, refused calls
    History('r16-f32-big-batch', 'R16-imgc3-ch12-20-8', [fwd(4), BWD, fwd(3, 2)], sprobe('f32')),
    History('r16-f16-noise-backward', 'R16-imgc3-ch12-20-8', [prec('f16x2'), fwd(4, 2), NBWD], sprobe('f16x2')),
    History('r16-bf16-refused-forward', 'R16-imgc3-ch12-20-8', [prec('bf16x3'), fwd(3), REF_FWD, BWD], sprobe('bf16x3')),
    History('r16-precision-after-forward', 'R16-imgc3-ch12-20-8', [prec('f16x2'), fwd(2), prec('f32'), BWD], sprobe('f32')),
    History('r16-precision-after-forward-2', 'R16-imgc3-ch12-20-8', [fwd(4), prec('f16x2'), NBWD], sprobe('f16x2')),
    History('shrink-f16-w-space', 'synth-shrinking-batch', [prec('f16x2'), fwd(4, 1, False), BWD, fwd(1, 0, True, False)], sprobe('f16x2')),
    History('shrink-bf16-equal-batch', 'synth-shrinking-batch', [prec('bf16x3'), fwd(2), NBWD, fwd(2)], sprobe('bf16x3')),
    History('shrink-f32-no-backward', 'synth-shrinking-batch', [fwd(4, 1, True, False), fwd(1), REF_FWD], sprobe('f16x2')),
]


def _pairs(values):
    return [(a, b) for a in values for b in values]


REQUIRED = {'synth': {
    'win': _pairs(WINS), 'prec': _pairs(MODES), 'sched': _pairs((0, 1)),
    'last': [(v, 'probe') for v in ('none', 'bwd', 'nbwd')], 'brel': [(v, 'probe') for v in ('larger', 'equal', 'smaller')],
    'win>prec': [(w, p) for w in WINS for p in MODES], 'prec>win': [(p, w) for p in MODES for w in WINS]}}


def synth_model_after(h):
    m = SynthModel()
    for op in h.ops:
        m.apply(op)
    return m


def _synth_pairs(h):
    s, p = synth_model_after(h).state(h.probe['B']), h.probe
    assert s['brel'] is not None, f'{h.name}: no forward pass in the history'
    return {'win': (s['win'], probe_win(p)), 'prec': (s['prec'], p['prec']), 'sched': (s['sched'], p['sched']), 'last': (s['last'], 'probe'),
            'brel': (s['brel'], 'probe'), 'win>prec': (s['win'], p['prec']), 'prec>win': (s['prec'], probe_win(p))}


# ---------------------------------------------------------------------------------------------------------------------------------
# discriminator and feature engine
#   state classes: prec x last, last = 'fwd' | 'loss' | 'bwd' | 'acc' (discriminator), 'fwd' | 'bwd' | 'pair' (feature engine).  The probe is a
#   whole pass in the precision the history left, or in another (probe['prec']): pairs (prec before, prec of the probe) and every `last`.

DISC_SHAPES = {'group-B3': 3, 'imgc3': 4}          # engine_cases.DISC_BY_NAME: the probe's batch (max_batch 4 in every engine here)
FEAT_SHAPES = {'conv-conv': 3, 'conv-conv-conv-pool': 3}


class EngineModel:
    def __init__(self, kind):
        self.kind, self.prec, self.last, self.lastB, self.passes = kind, 'f32', None, None, 0

    def valid(self, op):
        name = op[0]
        if name in ('loss', 'backward'):
            return self.last not in (None, 'pair')
        if name == 'refused_backward':          # feature engine: a backward behind pair_distance
            return self.kind == 'feat' and self.last == 'pair'
        return True

    def apply(self, op):
        name = op[0]
        assert self.valid(op), (op, vars(self))
        if name == 'forward':
            self.last, self.lastB = 'fwd', op[1]
            self.passes += 1
        elif name == 'loss':
            self.last = 'loss'
        elif name == 'backward':
            self.last = 'acc' if (self.kind == 'disc' and op[1]) else 'bwd'
        elif name == 'pair_distance':
            self.last = 'pair'
            self.passes += 1
        elif name == 'set_precision':
            self.prec = op[1]
        elif name in ('refused_forward', 'refused_backward'):
            return LA_ERR_ARG
        else:
            raise ValueError(name)
        return LA_OK

    def state(self):
        return dict(prec=self.prec, last=self.last)


def dfwd(B):
    return ('forward', B)


LOSS, DBWD, DACC, FBWD, REF_BWD = ('loss',), ('backward', 0), ('backward', 1), ('backward', 0), ('refused_backward',)


def pair(P):
    return ('pair_distance', P)


def eprobe(prec):
    return dict(prec=prec)


PAIRWISE['disc'] = [
    History('d-f32-f32', 'group-B3', [dfwd(4), LOSS, DBWD], eprobe('f32')),
    History('d-f32-bf16', 'group-B3', [dfwd(2), LOSS, DACC], eprobe('bf16x3')),
    History('d-f32-f16', 'imgc3', [dfwd(4), DBWD, dfwd(1)], eprobe('f16x2')),
    History('d-bf16-f32', 'imgc3', [prec('bf16x3'), dfwd(3), LOSS, DBWD], eprobe('f32')),
    History('d-bf16-bf16', 'group-B3', [prec('bf16x3'), dfwd(4), LOSS], eprobe('bf16x3')),
    History('d-bf16-f16', 'group-B3', [prec('bf16x3'), dfwd(1), DACC, REF_FWD], eprobe('f16x2')),
    History('d-f16-f32', 'group-B3', [prec('f16x2'), dfwd(4), LOSS, DBWD], eprobe('f32')),
    History('d-f16-bf16', 'imgc3', [prec('f16x2'), dfwd(2), DBWD, DACC], eprobe('bf16x3')),
    History('d-f16-f16-shrinking', 'imgc3', [prec('f16x2'), dfwd(4), LOSS, DBWD, dfwd(1), DBWD], eprobe('f16x2')),
    # suspect 1 of the issue: a setter between forward and backward (the backward runs in the forward's precision)
    History('d-set-f16-to-f32-mid-pass', 'imgc3', [prec('f16x2'), dfwd(4), prec('f32'), LOSS, DBWD], eprobe('f32')),
    History('d-set-f32-to-f16-mid-pass', 'group-B3', [dfwd(4), LOSS, prec('f16x2'), DACC], eprobe('f16x2')),
    History('d-set-bf16-to-f16-mid-pass', 'imgc3', [prec('bf16x3'), dfwd(3), prec('f16x2'), DBWD], eprobe('bf16x3')),
]
PAIRWISE['feat'] = [
    History('f-f32-f32', 'conv-conv', [dfwd(4), FBWD, dfwd(1)], eprobe('f32')),
    History('f-f32-bf16', 'conv-conv', [dfwd(2), FBWD, pair(2)], eprobe('bf16x3')),
    History('f-f32-f16', 'conv-conv-conv-pool', [dfwd(4), FBWD, FBWD], eprobe('f16x2')),
    History('f-bf16-f32', 'conv-conv-conv-pool', [prec('bf16x3'), dfwd(3), FBWD], eprobe('f32')),
    History('f-bf16-bf16', 'conv-conv', [prec('bf16x3'), pair(1), REF_BWD, dfwd(4)], eprobe('bf16x3')),
    History('f-bf16-f16', 'conv-conv', [prec('bf16x3'), dfwd(1), FBWD, REF_FWD], eprobe('f16x2')),
    History('f-f16-f32', 'conv-conv', [prec('f16x2'), dfwd(4), FBWD], eprobe('f32')),
    History('f-f16-bf16', 'conv-conv-conv-pool', [prec('f16x2'), dfwd(4), pair(2), REF_BWD], eprobe('bf16x3')),
    History('f-f16-f16-shrinking', 'conv-conv-conv-pool', [prec('f16x2'), dfwd(4), FBWD, dfwd(1), FBWD], eprobe('f16x2')),
    History('f-set-f16-to-f32-mid-pass', 'conv-conv-conv-pool', [prec('f16x2'), dfwd(4), prec('f32'), FBWD], eprobe('f32')),
    History('f-set-f32-to-f16-mid-pass', 'conv-conv', [dfwd(3), prec('f16x2'), FBWD], eprobe('f16x2')),
    History('f-set-bf16-to-f16-mid-pass', 'conv-conv-conv-pool', [prec('bf16x3'), dfwd(2), prec('f16x2'), FBWD, pair(1)], eprobe('bf16x3')),
]
REQUIRED['disc'] = {'prec': _pairs(MODES), 'last': [(v, 'probe') for v in ('fwd', 'loss', 'bwd', 'acc')]}
REQUIRED['feat'] = {'prec': _pairs(MODES), 'last': [(v, 'probe') for v in ('fwd', 'bwd', 'pair')]}


def engine_model_after(kind, h):
    m = EngineModel(kind)
    for op in h.ops:
        m.apply(op)
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# latent loop
#   The probe of a loop history is ONE run(B, losses asked or not, crop position) in whatever settings the history left (a probe that
#   applied setters would drop the captured step it is there to catch); the fresh stack gets the model's final settings after create.
#   state classes: graph = 'none' | 'fits' | 'stale' (a captured step exists and fits / does not fit the probe's key or settings) and
#   launch = 'replay' | 'eager' of the probe.

# crop: the case's own perceptual crop position (x, y), absolute (centre-crop offset added)
LOOP_SHAPES = {
    'all-R32': dict(R=32, max_batch=2, disc=True, feat=True, window=False, crop=(8, 16)),
    'all-W+-R32': dict(R=32, max_batch=2, disc=True, feat=True, window=False, crop=(8, 16)),
    'win-R64': dict(R=64, max_batch=2, disc=False, feat=True, window=True, crop=(19, 14)),               # pix + lpips
    'win-R128-cols': dict(R=128, max_batch=2, disc=False, feat=True, window=True, crop=(80, 64)),        # lpips alone: its window may leave the pixel criterion's crop
}
LOOP_STEPS = 3
LOOP_R128_CHANNELS = (8, 8, 4, 4, 4, 4)
LOOP_WIN_PREC = 'f16x2'          # (windows are planned in the 16-bit modes only)
FEAT_CROP = 8                    # loop_cases.FEAT_CROP


def crop_geometry(R):
    import math
    cc = int(math.sqrt(R * R / 2))
    return cc, int(round((R - cc) / 2.0))          # loop_cases.crop_geometry


# R = 128, lpips alone: two windows (rows, columns (70, 122)) and a perceptual crop position (x, y; absolute) inside each, outside the other
R128_WIN_A = dict(rows=(56, 80), cols=(70, 122), crop=(80, 64))
R128_WIN_B = dict(rows=(24, 44), cols=(70, 122), crop=(100, 30))


class LoopModel:
    """host-side state of a la_latent_opt handle and its attached engines, as far as the captured step depends on it"""

    def __init__(self, case, prec):
        sh = LOOP_SHAPES[case]
        self.case, self.sh = case, sh
        cc, off = crop_geometry(sh['R'])
        self.centre = (off, off + cc)
        self.rows = self.cols = self.centre if sh['window'] else (0, 0)          # LatentAug sets the centre crop as the loop window
        self.graph_mode, self.overlap, self.preproc, self.time_trace = 1, 2, 0, 0
        self.prec = dict(g=prec, d=prec, f=prec)
        self.sched = 0
        self.banks = 0          # generation of the bank contents
        self.graph = None       # key of the captured step: (B, windowed, parts, engine settings)
        self.crop = None        # absolute crop position of the last run

    def windowed(self, crop):
        sh = self.sh
        if self.rows[1] <= 0 or sh['disc']:
            return False

        def inside(y0, y1, x0, x1):
            return y0 >= self.rows[0] and y1 <= self.rows[1] and (self.cols[1] <= 0 or (x0 >= self.cols[0] and x1 <= self.cols[1]))
        ok = True
        if self.case == 'win-R64':          # the pixel criterion's centre crop
            ok = inside(self.centre[0], self.centre[1], self.centre[0], self.centre[1])
        return ok and inside(crop[1], crop[1] + FEAT_CROP, crop[0], crop[0] + FEAT_CROP)

    def key(self, B, crop):
        crop = self.sh['crop'] if crop is None else crop
        parts = 4 if (self.overlap == 1 and self.sh['disc'] and self.sh['feat']) else 1
        return (B, self.windowed(crop), parts, tuple(sorted(self.prec.items())), self.sched, self.rows, self.cols, self.preproc, self.overlap)

    def replayable(self, losses, trace):
        return self.graph_mode == 1 and not losses and not trace and LOOP_STEPS > 0

    def valid(self, op):
        return True

    def apply(self, op):
        name = op[0]
        if name == 'run':
            _, B, losses, trace, crop = op
            if self.replayable(losses, trace):
                self.graph = self.key(B, crop)
            self.crop = crop
        elif name == 'refused_run':
            return LA_ERR_ARG
        elif name == 'set_graph':
            self.graph_mode = op[1]
            if not op[1]:
                self.graph = None
        elif name == 'set_overlap':
            self.overlap, self.graph = op[1], None
        elif name == 'set_rows':
            if tuple(op[1:3]) != self.rows:
                self.graph = None
            self.rows = tuple(op[1:3])
        elif name == 'set_cols':
            if tuple(op[1:3]) != self.cols:
                self.graph = None
            self.cols = tuple(op[1:3])
        elif name == 'set_time_trace':
            self.time_trace = op[1]
        elif name == 'set_preproc':
            self.preproc, self.graph = op[1], None
        elif name == 'engine_precision':          # ('engine_precision', 'g' | 'd' | 'f', mode) on the ATTACHED engine
            self.prec[op[1]] = op[2]
        elif name == 'engine_schedule':
            self.sched = op[1]
        elif name == 'invalidate_banks':          # rewrite the three banks in place with the next seeded values, then the call
            self.banks += 1
        else:
            raise ValueError(name)
        return LA_OK

    def graph_state_after(self, B, losses, trace, crop):
        """what la_latent_opt_graph_state must say after the probe: 1 after a replayable run; an eager run leaves what was there"""
        return 1 if (self.replayable(losses, trace) or self.graph is not None) else 0

    def state(self, probe):
        _, B, losses, trace, crop = probe
        launch = 'replay' if self.replayable(losses, trace) else 'eager'
        graph = 'none' if self.graph is None else ('fits' if self.graph == self.key(B, crop) else 'stale')
        return dict(graph=graph, launch=launch)


def run(B, losses=False, trace=None, crop=None):
    """run(B, losses asked, trace None | 'w' | 'w+img' | 'grad', absolute crop position (x, y) or None = the case's)"""
    return ('run', B, bool(losses), trace, crop)


def lprobe(B, losses=False, crop=None, prec='f32'):
    return dict(run=run(B, losses, None, crop), prec=prec)


REF_RUN = ('refused_run',)
INVALIDATE = ('invalidate_banks',)


def eng_prec(which, mode):
    return ('engine_precision', which, mode)


A, Bw = R128_WIN_A, R128_WIN_B
PAIRWISE['loop'] = [
    # eager -> captured -> eager -> replay (traces on for a run, then off)
    History('trace-capture-trace-replay', 'all-R32', [run(2, trace='w+img'), run(2), run(2, trace='grad')], lprobe(2)),
    History('losses-then-replay-other-batch', 'all-R32', [run(2, True), run(2), run(1), REF_RUN], lprobe(2)),
    History('time-trace-and-losses', 'all-W+-R32', [('set_time_trace', 1), run(2, True), ('set_time_trace', 0), run(1)], lprobe(2, True)),
    History('graph-off-and-on', 'all-W+-R32', [run(2), ('set_graph', 0), run(2), ('set_graph', 1)], lprobe(2)),
    History('graph-off-probe-eager', 'all-R32', [run(1), run(2), ('set_graph', 0)], lprobe(2)),
    History('overlap-modes', 'all-R32', [run(2), ('set_overlap', 1), run(2), ('set_overlap', 0), run(1), ('set_overlap', 2)], lprobe(2)),
    History('overlap-split-replay-probe', 'all-W+-R32', [run(2), ('set_overlap', 1), run(1)], lprobe(2)),
    History('preproc-changed-and-back', 'all-R32', [run(2), ('set_preproc', 1), run(2), ('set_preproc', 0)], lprobe(2)),
    # suspect 2 of the issue: setters of the ATTACHED engines between replaying runs
    History('synth-precision-between-runs', 'all-R32', [run(2), eng_prec('g', 'f16x2'), run(2), eng_prec('g', 'f32')], lprobe(2)),
    History('synth-precision-stays-changed', 'all-R32', [run(2), run(2), eng_prec('g', 'bf16x3')], lprobe(2)),
    History('disc-precision-stays-changed', 'all-W+-R32', [run(2), run(2), eng_prec('d', 'f16x2')], lprobe(2)),
    History('feat-precision-stays-changed', 'all-R32', [run(2), run(2), eng_prec('f', 'f16x2')], lprobe(2)),
    History('all-precisions-changed-and-back', 'all-W+-R32', [eng_prec('g', 'f16x2'), eng_prec('d', 'f16x2'), eng_prec('f', 'f16x2'), run(2), eng_prec('g', 'f32'),
                                                             eng_prec('d', 'f32')], lprobe(2)),
    History('schedule-changed', 'all-R32', [run(2), ('engine_schedule', 1), run(1)], lprobe(2)),
    History('schedule-stays-changed', 'all-R32', [run(2), run(2), ('engine_schedule', 1)], lprobe(2)),
    # the column sums of rewritten banks (la_latent_opt_invalidate_banks)
    History('banks-rewritten', 'all-R32', [run(2), run(2, True), INVALIDATE], lprobe(2, True)),
    History('banks-rewritten-replay', 'all-W+-R32', [run(2), run(1), INVALIDATE], lprobe(2)),
    # the loop window at 64^2 (pix + lpips): set, moved so that it no longer covers the criteria, cleared, set again
    History('win64-replay-after-whole-frames', 'win-R64', [run(2), ('set_rows', 0, 0), run(2), ('set_rows', 10, 55)], lprobe(2, prec=LOOP_WIN_PREC)),
    History('win64-window-too-small', 'win-R64', [run(2), ('set_rows', 20, 40), run(2), ('set_rows', 8, 60), run(1)], lprobe(2, prec=LOOP_WIN_PREC)),
    History('win64-crop-leaves-the-window', 'win-R64', [run(2), run(2, crop=(2, 2)), run(1, trace='w')], lprobe(2, prec=LOOP_WIN_PREC)),
    History('win64-synth-precision-changed', 'win-R64', [run(2), run(2), eng_prec('g', 'bf16x3')], lprobe(2, prec=LOOP_WIN_PREC)),
    # rows and the columns (70, 122) at 128^2 (lpips alone): the window moves with the crop
    History('win128-window-moves-with-the-crop', 'win-R128-cols', [('set_rows', *A['rows']), ('set_cols', *A['cols']), run(2, crop=A['crop']), run(2, crop=A['crop']),
                                                                  ('set_rows', *Bw['rows'])], lprobe(2, crop=Bw['crop'], prec=LOOP_WIN_PREC)),
    History('win128-crop-outside-then-inside', 'win-R128-cols', [('set_rows', *A['rows']), ('set_cols', *A['cols']), run(2, crop=Bw['crop']), run(1, crop=A['crop'])],
            lprobe(2, crop=A['crop'], prec=LOOP_WIN_PREC)),
    History('win128-cols-cleared', 'win-R128-cols', [('set_rows', *A['rows']), ('set_cols', *A['cols']), run(2, crop=A['crop']), ('set_cols', 0, 0), run(2, True, crop=A['crop'])],
            lprobe(2, crop=A['crop'], prec=LOOP_WIN_PREC)),
]
del A, Bw
REQUIRED['loop'] = {'graph>launch': [(g, l) for g in ('none', 'fits', 'stale') for l in ('replay', 'eager')]}


def loop_model_after(h):
    m = LoopModel(h.case, h.probe['prec'])
    for op in h.ops:
        m.apply(op)
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# reach and the random histories

def pairs_of(kind, h):
    if kind == 'synth':
        return _synth_pairs(h)
    if kind in ('disc', 'feat'):
        s = engine_model_after(kind, h).state()
        return {'prec': (s['prec'], h.probe['prec']), 'last': (s['last'], 'probe')}
    s = loop_model_after(h).state(h.probe['run'])
    return {'graph>launch': (s['graph'], s['launch'])}


def reach(kind, histories=None):
    """{axis: {(before, probe): [names of the histories that have the pair]}} over PAIRWISE[kind]"""
    table = {axis: {p: [] for p in want} for axis, want in REQUIRED[kind].items()}
    for h in (PAIRWISE[kind] if histories is None else histories):
        for axis, p in pairs_of(kind, h).items():
            table[axis].setdefault(p, []).append(h.name)
    return table


def reach_text(kind):
    lines = []
    for axis, row in reach(kind).items():
        for p, names in row.items():
            lines.append(f'    {kind} {axis} {p[0]} -> {p[1]}: ' + (', '.join(names) if names else 'NO HISTORY'))
    return '\n'.join(lines)


RANDOM_SEEDS = {'synth': [101, 102, 103, 104, 105, 106, 107, 108], 'disc': [201, 202, 203, 204, 205, 206, 207, 208],
                'feat': [301, 302, 303, 304, 305, 306, 307, 308], 'loop': [401, 402, 403, 404, 405, 406, 407, 408]}


def _synth_candidates(rng, sh):
    R = sh['R']
    ops = [fwd(rng.randint(1, MAX_BATCH), rng.randint(0, 2), rng.random() < 0.7, rng.random() < 0.7), fwd(rng.randint(1, MAX_BATCH)), BWD, BWD, NBWD,
           prec(rng.choice(MODES)), REF_FWD]
    if R >= 64:
        ops.append(sched(rng.randint(0, 1)))
    if sh['rows']:
        ops += [rows(*rng.choice(sh['rows'])), CLEAR, REF_NOISE]
    if sh['cols']:
        ops.append(cols(*rng.choice(sh['cols'])))
    return ops


def _engine_candidates(kind, rng):
    ops = [dfwd(rng.randint(1, MAX_BATCH)), dfwd(rng.randint(1, MAX_BATCH)), prec(rng.choice(MODES)), REF_FWD]
    return ops + ([LOSS, DBWD, DACC] if kind == 'disc' else [FBWD, FBWD, pair(rng.randint(1, 2)), REF_BWD])


def _loop_candidates(rng, case):
    sh = LOOP_SHAPES[case]
    ops = [run(rng.randint(1, sh['max_batch']), rng.random() < 0.3, rng.choice([None, None, 'w', 'w+img', 'grad'])), run(rng.randint(1, sh['max_batch'])),
           ('set_graph', rng.randint(0, 1)), ('set_overlap', rng.randint(0, 2)), ('set_time_trace', rng.randint(0, 1)), ('set_preproc', rng.randint(0, 1)),
           eng_prec(rng.choice('gf' + ('d' if sh['disc'] else '')), rng.choice(MODES[1:] if sh['window'] else MODES)), ('engine_schedule', rng.randint(0, 1)), REF_RUN,
           INVALIDATE]
    if case == 'win-R64':
        ops += [('set_rows', *rng.choice([(0, 0), (10, 55), (8, 60), (20, 40)]))]
    return ops


def random_history(kind, seed):
    rng = random.Random(seed)
    n = rng.randint(LEN_MIN, LEN_MAX)
    if kind == 'synth':
        case = rng.choice(sorted(SYNTH_SHAPES))
        sh, model = SYNTH_SHAPES[case], SynthModel()
        pr = sprobe(rng.choice(MODES), rng.randint(0, 1) if sh['R'] >= 64 else 0)
        if sh['rows'] and rng.random() < 0.6:
            pr['rows'] = tuple(rng.choice(sh['rows']))
            if sh['cols'] and rng.random() < 0.5:
                pr['cols'] = tuple(rng.choice(sh['cols']))
        cand = lambda: _synth_candidates(rng, sh)          # noqa: E731
        must = lambda: fwd(rng.randint(1, MAX_BATCH))      # noqa: E731
    elif kind in ('disc', 'feat'):
        case = rng.choice(sorted(DISC_SHAPES if kind == 'disc' else FEAT_SHAPES))
        model, pr = EngineModel(kind), eprobe(rng.choice(MODES))
        cand = lambda: _engine_candidates(kind, rng)       # noqa: E731
        must = lambda: dfwd(rng.randint(1, MAX_BATCH))     # noqa: E731
    else:
        case = rng.choice(['all-R32', 'all-W+-R32', 'win-R64'])
        p = LOOP_WIN_PREC if LOOP_SHAPES[case]['window'] else rng.choice(MODES)
        model, pr = LoopModel(case, p), lprobe(rng.randint(1, LOOP_SHAPES[case]['max_batch']), rng.random() < 0.3, prec=p)
        cand = lambda: _loop_candidates(rng, case)         # noqa: E731
        must = lambda: run(rng.randint(1, LOOP_SHAPES[case]['max_batch']))                          # noqa: E731
    ops, ran = [], False
    for i in range(n):
        if i == n - 1 and not ran:          # (every history has a pass)
            op = must()
        else:
            op = rng.choice([o for o in cand() if model.valid(o)])
        ran = ran or op[0] in ('forward', 'run')
        model.apply(op)
        ops.append(op)
    return History(f'random-{seed}', case, ops, pr)


RANDOM = {kind: [random_history(kind, s) for s in seeds] for kind, seeds in RANDOM_SEEDS.items()}


def all_histories(kind):
    return PAIRWISE[kind] + RANDOM[kind]


if __name__ == '__main__':
    for k in ('synth', 'disc', 'feat', 'loop'):
        print(reach_text(k))
        for hh in RANDOM[k]:
            print('   ', hh)
