"""Which library call a step is: the launch KINDS, `candidates` — the ordered kinds an env's options allow, a pure function —, and
StepPlan, which walks them at an env's first step, remembers the first the library accepts and makes that call from then on
(MultiGridEnv._launch_step delegates here).  A refusal — MG_E_UNSUPPORTED: nothing was launched, the next
candidate is tried in the same step — is kept in ONE set for the env's life: the library refuses by shape, LDS and table size
and the object registry only grows, so a "no" cannot become a "yes"; the delta's signature tensors are freed at its refusal,
since step() must allocate nothing.  The remembered choice (not the refusals) is dropped by _release_spec() — the `specialize`
handles are new objects then — and by an assignment to env.encode_in_step: the step may be another call afterwards."""
import ctypes as C
import functools
from collections import namedtuple

from . import _native as N

# call: the library's entry point (None: this env has no such call, only its demand speaks); args(env, ep, stream): what follows
# the head every call shares; encodes: it writes grid_encoding (else mg_encode follows where encode_in_step asks); demand: a kind
# obs_delta=True requires — the NotImplementedError text of its refusal; follows: the views are launched behind it, one per group;
# latch: the name its refusal is kept under (None: MG_E_UNSUPPORTED is an error like any other; "delta": it needs the signatures
# and counts in env._delta_launches); want: the `specialize` handle it is called through
Kind = namedtuple("Kind", "call args encodes demand follows latch want", defaults=(False, None, False, None, None))

_NO_DELTA = ("obs_delta=True needs the fused image step without view groups, and a shape the library "
             "has a delta instantiation for (view 7 at 8-pixel tiles, at most 3 agents, no 'prestige' agent)")
_NO_DELTA_EX = ("obs_delta=True with %s: no delta launch for this configuration — it needs the fused image step "
                "(fused_step=True, obs_format='image', one view group), view 7 at 8-pixel tiles, at most 3 agents, "
                "no 'prestige' agent, grid and atlas in LDS, and for encode_in_step at most 256 object kinds + agent marks")
_obs = lambda e, ep, s: (e.obs.data_ptr(), s)
_obs_ep = lambda e, ep, s: (e.obs.data_ptr(), ep, s)
_sig = lambda e: e._ring[e._ring_i]["sig"].data_ptr()       # (whether a band is stored is decided on the device, against it)
_enc = lambda e: e._encoding_buffer().data_ptr()

RENDER = Kind("mg_step_render", _obs)
RENDER_EP = Kind("mg_step_render_ep", _obs_ep, latch="ep")
RENDER_ENCODE = Kind("mg_step_render_encode", lambda e, ep, s: (e.obs.data_ptr(), _enc(e), s), encodes=True, latch="enc")
DELTA = Kind("mg_step_render_delta", lambda e, ep, s: (e.obs.data_ptr(), _sig(e), 0, s), latch="delta")
DELTA_DEMAND = DELTA._replace(demand=_NO_DELTA)
# the delta with episode outputs, the grid encoding or both: the same body, other arguments, always a demand ("auto" never asks)
DELTA_EX_EP = Kind("mg_step_render_delta_ex", lambda e, ep, s: (e.obs.data_ptr(), _sig(e), 0, None, ep, s),
                   demand=_NO_DELTA_EX % "episode outputs", latch="delta")
DELTA_EX_ENCODE = DELTA_EX_EP._replace(args=lambda e, ep, s: (e.obs.data_ptr(), _sig(e), 0, _enc(e), ep, s), encodes=True,
                                       demand=_NO_DELTA_EX % "encode_in_step")
DELTA_EX_BOTH = DELTA_EX_ENCODE._replace(demand=_NO_DELTA_EX % "episode outputs + encode_in_step")
SPEC = Kind("mg_step_render_spec", lambda e, ep, s: (e.obs.data_ptr(), None, None, s), want=N.WANT_PLAIN)
SPEC_ENCODE = SPEC._replace(args=lambda e, ep, s: (e.obs.data_ptr(), _enc(e), None, s), encodes=True, want=N.WANT_ENCODE)
SPEC_EP = SPEC._replace(args=lambda e, ep, s: (e.obs.data_ptr(), None, ep, s), want=N.WANT_EPISODE)
ENCODE_VIEWS = Kind("mg_step_encode_views", _obs)
ENCODE_VIEWS_EP = Kind("mg_step_encode_views_ep", _obs_ep)
TWO = Kind("mg_step", lambda e, ep, s: (s,), follows=True)
TWO_EP = Kind("mg_step_ep", lambda e, ep, s: (ep, s), follows=True)


def candidates(obs_delta, use_ep, encode_in_step, fused_step, hetero, encoded, spec):
    """The kinds this env's step can be, in the order they are tried.  `spec(want)`: the first view group's `specialize` handle
    or None — asked only for the wants, and in the order, a step needs them (asking may compile)."""
    fused = fused_step and not hetero
    if obs_delta is True and (use_ep or encode_in_step):
        kind = DELTA_EX_BOTH if use_ep and encode_in_step else DELTA_EX_EP if use_ep else DELTA_EX_ENCODE
        return [kind if fused and not encoded else kind._replace(call=None)]
    if not fused:
        return [TWO_EP if use_ep else TWO]
    if encoded:
        return [ENCODE_VIEWS_EP if use_ep else ENCODE_VIEWS]
    if use_ep:      # (there is no _ep twin of mg_step_render_encode: encode_in_step takes mg_step_render_ep + mg_encode)
        return [SPEC_EP] if spec(N.WANT_EPISODE) else [RENDER_EP, TWO_EP]
    if encode_in_step and spec(N.WANT_ENCODE):
        return [SPEC_ENCODE]
    first = [RENDER_ENCODE] if encode_in_step else []
    h = spec(N.WANT_PLAIN)
    if obs_delta is True:       # (obs_delta keeps the table's path: its one shape is on the table)
        return [DELTA_DEMAND]
    if h:
        return first + [SPEC]
    return first + ([DELTA] if obs_delta == "auto" and not encode_in_step else []) + [RENDER]


class StepPlan:
    def __init__(self):
        self.refused = set()        # latches of the kinds the library answered MG_E_UNSUPPORTED for
        self.chosen = None          # (kind, its call — bound to the handle, if any —, a delta, mg_encode follows): the accepted one

    def delta_wanted(self, e):      # a step that has a delta twin, and the library has not said no ("auto": the plain step alone)
        return (e.obs_delta is not False and "delta" not in self.refused and not e._encoded and e.fused_step and not e._hetero
                and (e.obs_delta is True or not (e._use_ep or e.encode_in_step)))

    def launch(self, e, actions, prog, stream, probe, ep):
        """the step and its observations; then the views, where the kind leaves them to follow, and mg_encode unless the call encoded"""
        head = (C.byref(e._cfg), C.byref(e._state), actions.data_ptr(), actions.element_size(), e.rewards.data_ptr(), prog)
        chosen = self.chosen
        if chosen is None:
            rc, chosen = self._resolve(e, head, ep, stream), self.chosen
        else:
            rc = chosen[1](*head, *chosen[0].args(e, ep, stream))
        kind, _, delta, encode_behind = chosen
        if delta:
            e._delta_launches += 1
        if rc:
            N.check(rc)
        if kind.follows:
            if probe is not None:
                probe(1)
            e._launch_views()
        if encode_behind:
            e._encode_into(e._encoding_buffer())

    def _resolve(self, e, head, ep, stream):
        g = e._groups[0]        # walk the candidates: make the first call the library accepts and remember it
        for kind in candidates(e.obs_delta, ep is not None, e.encode_in_step, e.fused_step, e._hetero, e._encoded, lambda w: e._spec(g, w)):
            delta = kind.latch == "delta"
            if kind.call and kind.latch not in self.refused and not (delta and e._ring[e._ring_i]["sig"] is None):
                call = getattr(e._lib, kind.call)
                if kind.want is not None:
                    call = functools.partial(call, g.spec[kind.want])
                rc = call(*head, *kind.args(e, ep, stream))
                if rc != N.E_UNSUPPORTED or kind.latch is None:
                    self.chosen = (kind, call, delta, e.encode_in_step and not kind.encodes)
                    return rc
                self.refused.add(kind.latch)        # (nothing was launched)
                for r in e._ring if delta else ():
                    r["sig"] = None
            if kind.demand:
                raise NotImplementedError(kind.demand)
