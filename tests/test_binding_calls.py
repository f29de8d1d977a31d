"""The Python binding's calls into the C ABI (copra_amd/batch.py over include/copra_hip.h), without a GPU: _capi.lib is replaced by a recorder
whose every attribute is a function that notes its name and arguments and returns 0.

A. A fixed script of numpy calls -- every setter in every accepted shape form, and every refusal made before the library is called -- produces
   the record in tests/golden/binding_calls.json (written by this file's __main__ from the binding as it was before copra_amd/_args.py
   existed; `PYTHONPATH=. python tests/test_binding_calls.py` writes it again): function names, scalars, and the BYTES every array argument
   points to at the time of the call.
B. The device path: with the residency predicate replaced, CPU float64 tensors go the way of CUDA tensors -- the pointers are data_ptr(), the
   flags those of the equivalent numpy call, and the keep-alive registry holds and releases them as its table says.
C. The two shape rules, form by form.
D. (gpu) the refusals with real CUDA tensors leave a controller solving to the same bits as a twin that never saw them.

The element count of every array below is written from the comments of include/copra_hip.h, not from the binding."""
import ctypes as C
import gc
import json
import os
import weakref

import numpy as np
import pytest

from copra_amd import _capi
from copra_amd import batch as batch_mod

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_calls.json")
NX, NU, N, NY = 4, 2, 3, 2
BATCHES = (5, 4, 2)  # 4 == nx and 2 == nu: the tie rule of the weight forms
OUT = "out"  # an array the library writes: noted as given / not given


def _per(d, a):
    return d.b if a["per_instance"] else 1


# function -> [(argument, None: a scalar | OUT | element count (d: the controller's sizes, a: the call's own arguments))], after the handle
F = {
    "copra_batch_set_system": [("A", lambda d, a: d.b * NX * NX), ("B", lambda d, a: d.b * NX * NU), ("d", lambda d, a: d.b * NX),
                               ("x0", lambda d, a: d.b * NX), ("on_device", None)],
    "copra_batch_set_system_rowmajor_async": [("A", lambda d, a: d.b * NX * NX), ("B", lambda d, a: d.b * NX * NU), ("d", lambda d, a: d.b * NX),
                                              ("x0", lambda d, a: d.b * NX), ("hip_stream", None)],
    "copra_batch_set_x0": [("x0", lambda d, a: d.b * NX), ("on_device", None)],
    "copra_batch_set_shared_system": [("A", lambda d, a: NX * NX), ("B", lambda d, a: NX * NU), ("d", lambda d, a: NX), ("on_device", None)],
    "copra_batch_set_cost_reference": [("cost_index", None), ("p", lambda d, a: d.b * d.cost_rows[a["cost_index"]]), ("on_device", None)],
    "copra_batch_set_cost_reference_all": [("cost_index", None), ("p", lambda d, a: d.cost_rows[a["cost_index"]]), ("on_device", None)],
    "copra_batch_set_cost_weights": [("cost_index", None), ("w", lambda d, a: d.b * d.cost_rows[a["cost_index"]]), ("on_device", None)],
    "copra_batch_set_constraint_rhs": [("cstr_index", None), ("f", lambda d, a: d.b * d.cstr_rows[a["cstr_index"]]), ("on_device", None)],
    "copra_batch_set_control_bounds": [("lower", lambda d, a: d.b * NU * N), ("upper", lambda d, a: d.b * NU * N), ("on_device", None)],
    "copra_batch_set_initial_state_bounds": [("x0lb", lambda d, a: d.b * NX), ("x0ub", lambda d, a: d.b * NX), ("on_device", None)],
    "copra_batch_set_outputs": [("control", OUT), ("trajectory", OUT), ("status", OUT), ("iter", OUT)],
    "copra_batch_solve": [("hip_stream", None)],
    "copra_batch_set_reference_schedule": [("cost_index", None), ("sched", lambda d, a: _per(d, a) * a["steps"] * a["r"]), ("steps", None), ("r", None),
                                           ("offset", None), ("per_instance", None), ("on_device", None)],
    "copra_batch_set_constraint_schedule": [("cstr_index", None), ("sched", lambda d, a: _per(d, a) * a["steps"] * a["r"]), ("steps", None), ("r", None),
                                            ("offset", None), ("preview", None), ("per_instance", None), ("on_device", None)],
    "copra_batch_set_control_bound_schedule": [("lower", lambda d, a: _per(d, a) * a["steps"] * NU), ("upper", lambda d, a: _per(d, a) * a["steps"] * NU),
                                               ("steps", None), ("offset", None), ("preview", None), ("per_instance", None), ("on_device", None)],
    "copra_batch_set_bias_estimator": [("gain", lambda d, a: _per(d, a) * NX * (NX if a["dense"] else 1)), ("dense", None), ("per_instance", None),
                                       ("on_device", None)],
    "copra_batch_set_bias": [("d", lambda d, a: d.b * NX), ("on_device", None)],
    "copra_batch_set_plant_state": [("x", lambda d, a: d.b * NX), ("on_device", None)],
    "copra_batch_set_observer": [("ny", None), ("C", lambda d, a: _per(d, a) * a["ny"] * NX), ("Lx", lambda d, a: _per(d, a) * a["ny"] * NX),
                                 ("Ld", lambda d, a: _per(d, a) * a["ny"] * NX), ("per_instance", None), ("on_device", None)],
    "copra_batch_draw_noise": [("tick", None), ("stream", None), ("out_device", OUT), ("hip_stream", None)],
    "copra_batch_set_noise": [("noise", "Noise")],
    "copra_batch_set_score": [("score", "Score")],
    "copra_batch_set_target": [("target", "Target")],
    "copra_batch_advance": [("step", "PlantStepObs"), ("hip_stream", None)],
    "copra_batch_rollout": [("step", "PlantStepObs"), ("ticks", None), ("w_seq", lambda d, a: a["ticks"] * d.b * NX), ("x_hist", OUT), ("u_hist", OUT),
                            ("status_hist", OUT), ("hip_stream", None)],
}


def _plant(rows, cols):
    return lambda d, s, a: (1 if s.shared else d.b) * rows * cols


# struct -> {pointer field: OUT | element count (d, s: the struct, a: the call's arguments)}
S = {
    "Noise": {"sigma_w": lambda d, s, a: _per(d, dict(per_instance=s.per_instance)) * NX,
              "sigma_v": lambda d, s, a: _per(d, dict(per_instance=s.per_instance)) * d.ny},
    "Score": dict({"qx": lambda d, s, a: (d.b if s.per_instance else 1) * NX * (NX if s.dense else 1),
                   "ru": lambda d, s, a: (d.b if s.per_instance else 1) * NU * (NU if s.dense else 1),
                   "x_ref": lambda d, s, a: (d.b if s.per_instance else 1) * s.ref_steps * NX},
                  **{k: (lambda d, s, a: (d.b if s.per_instance else 1) * NX) for k in ("x_lo", "x_hi")},
                  **{k: (lambda d, s, a: (d.b if s.per_instance else 1) * NU) for k in ("u_lo", "u_hi")}),
    "Target": {"H": lambda d, s, a: s.nr * NX, "r": lambda d, s, a: (d.b if s.per_instance else 1) * s.steps * s.nr},
    "PlantStepObs": dict({"A": _plant(NX, NX), "B": _plant(NX, NU), "d": _plant(NX, 1), "w": lambda d, s, a: d.b * NX,
                          "fallback_u": lambda d, s, a: d.b * NU, "v": lambda d, s, a: d.b * d.ny, "y_meas": lambda d, s, a: d.b * d.ny,
                          "v_seq": lambda d, s, a: a["ticks"] * d.b * d.ny},
                         **{k: OUT for k in ("x_out", "u_out", "status_out", "age_out", "age_hist", "d_out", "d_hist", "y_out", "xhat_out", "y_hist",
                                             "xhat_hist")}),
}
UNRECORDED = ("copra_batch_destroy", "copra_last_error")


def _bytes(ptr, count, itemsize=8):
    return C.string_at(ptr, count * itemsize).hex()


class Recorder:
    """stands in for libcopra_hip.so: .calls is the record, .raw the pointers of the same calls as they were passed; a function named in
    .refuse returns COPRA_ERR_ARG"""

    def __init__(self):
        self.calls, self.raw, self.refuse = [], [], set()
        self.b = self.ny = 0
        self.cost_rows, self.cstr_rows = [], []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name == "copra_last_error":
            return lambda: b"refused by the recorder"

        def fn(*args):
            if name in UNRECORDED:
                return 0
            self._note(name, args)
            return _capi.COPRA_ERR_ARG if name in self.refuse else 0
        return fn

    @staticmethod
    def _scalar(v):
        if v is None:
            return "null"
        if isinstance(v, C.c_void_p):
            return "handle" if v.value else "null"
        if type(v).__name__ == "CArgObject":
            return OUT
        if isinstance(v, (bytes, C._CFuncPtr)):
            return "given"
        return v

    def _array(self, ptr, size, raw, key, *ctx):
        raw[key] = ptr
        if not ptr:
            return "null"
        return "given" if size is OUT else _bytes(ptr, size(self, *ctx))

    def _struct(self, st, kind, a, raw):
        out = {}
        for f, _ in st._fields_:
            v = getattr(st, f)
            if f in S[kind]:
                out[f] = self._array(v, S[kind][f], raw, f, st, a)
            elif kind == "Target" and f in ("cost_index", "cost_rows"):
                out[f] = [v[i] for i in range(st.n_costs)]
            elif kind == "Target" and f == "cost_map":
                raw[f] = [v[i] for i in range(st.n_costs)]
                out[f] = [_bytes(v[i], st.cost_rows[i] * (NX + NU)) for i in range(st.n_costs)]
            else:
                out[f] = v
        return out

    def _note(self, name, args):
        raw = {}
        if name == "copra_batch_create_with_options":  # (out, dims, n_costs, costs, n_cstrs, cstrs, initial_state, options)
            dims = args[1]._obj
            self.b = dims.batch
            self.cost_rows = [args[3][i].rows for i in range(args[2])]
            self.cstr_rows = [args[5][i].rows for i in range(args[4])]
            entry = dict(dims=[dims.nx, dims.nu, dims.N, dims.batch], n_costs=args[2], n_cstrs=args[4])
        elif name in F:
            a = {nm: v for (nm, _), v in zip(F[name], args[1:])}
            assert len(a) == len(args) - 1, name
            entry = {}
            for nm, size in F[name]:
                v = a[nm]
                if isinstance(size, str) and size != OUT:
                    entry[nm] = "null" if v is None else self._struct(v._obj, size, a, raw)
                elif size is None:
                    entry[nm] = self._scalar(v)
                else:
                    entry[nm] = self._array(v, size, raw, nm, a)
            if name == "copra_batch_set_observer":
                self.ny = a["ny"]
            elif name == "copra_batch_set_shared_system":
                self.ny = 0  # (the library ends the observer)
        else:
            entry = {"a%d" % i: self._scalar(v) for i, v in enumerate(args[1:], 1)}
        self.calls.append(dict(fn=name, **entry))
        self.raw.append(raw)


def _costs():
    return [dict(kind="trajectory", M=np.eye(NX), p=np.zeros(NX), weights=np.ones(NX)),
            dict(kind="control", N=np.eye(NU), p=np.zeros(NU), weights=np.ones(NU)),
            dict(kind="target", M=np.arange(2.0 * NX).reshape(2, NX), p=np.zeros(2), weights=np.ones(2))]


def _cstrs():
    return [dict(kind="control", G=np.eye(NU), f=np.ones(NU)), dict(kind="control_bound", lower=-np.ones(NU), upper=np.ones(NU))]


def controller(monkeypatch_or_none, b):
    """(a BatchLMPC over a fresh Recorder, the recorder)"""
    rec = Recorder()
    if monkeypatch_or_none is None:
        _capi.lib = lambda: rec
    else:
        monkeypatch_or_none.setattr(_capi, "lib", lambda: rec)
    return batch_mod.BatchLMPC(NX, NU, N, b, _costs(), _cstrs()), rec


# ---- A. the script ----
def script(eng, b):
    """[(label, a call without arguments)]: numpy inputs only, from one seeded generator, in a fixed order"""
    rng = np.random.default_rng(20261021 + b)

    def A(*shape):
        return rng.standard_normal(shape)

    steps = []

    def add(label, fn, *args, **kw):
        steps.append((label, lambda: fn(*args, **kw)))

    add("system", eng.set_system, A(b, NX, NX), A(b, NX, NU), A(b, NX), A(b, NX))
    add("system float32", eng.set_system, A(b, NX, NX).astype(np.float32), A(b, NX, NU).astype(np.float32), A(b, NX).tolist(), A(b, NX))
    add("shared system", eng.set_shared_system, A(NX, NX), A(NX, NU), A(NX))
    add("x0", eng.set_x0, A(b, NX))
    add("x0 from a transposed view", eng.set_x0, A(NX, b).T)
    add("reference per instance", eng.set_cost_reference, 0, A(b, NX))
    add("reference for all", eng.set_cost_reference, 2, A(2))
    add("reference None", eng.set_cost_reference, 0, None)
    add("weights per instance", eng.set_cost_weights, 1, np.abs(A(b, NU)))
    add("weights for all", eng.set_cost_weights, 1, np.abs(A(NU)))
    add("weights None", eng.set_cost_weights, 1, None)
    add("weights: wrong rows", eng.set_cost_weights, 1, A(b, NU + 1))
    add("weights: wrong rows for all", eng.set_cost_weights, 1, A(NU + 1))
    add("constraint rhs", eng.set_constraint_rhs, 0, A(b, NU))
    add("control bounds scalars", eng.set_control_bounds, -1.5, 2)
    add("control bounds once and per instance", eng.set_control_bounds, A(NU * N), A(b, NU * N))
    add("control bounds: not broadcastable", eng.set_control_bounds, A(b, NU * N + 1), 1.0)
    add("initial state bounds", eng.set_initial_state_bounds, A(NX), A(b, NX))
    add("initial state bounds: not broadcastable", eng.set_initial_state_bounds, A(NX + 1), 0.0)
    # the signal rule
    add("reference schedule", eng.set_reference_schedule, 0, A(6, NX), NX)
    add("reference schedule per instance, offset", eng.set_reference_schedule, 0, A(b, 6, NX), NX, offset=2)
    add("reference schedule of batch steps", eng.set_reference_schedule, 2, A(b, 2), 2)
    add("reference schedule None", eng.set_reference_schedule, 0, None, NX)
    add("reference schedule: wrong r", eng.set_reference_schedule, 0, A(6, NX - 1), NX)
    add("reference schedule: wrong batch", eng.set_reference_schedule, 0, A(b + 1, 6, NX), NX)
    add("reference schedule: 1-d", eng.set_reference_schedule, 0, A(NX), NX)
    add("constraint schedule", eng.set_constraint_schedule, 0, A(6, NU), NU)
    add("constraint schedule per instance, offset, no preview", eng.set_constraint_schedule, 0, A(b, 7, NU), NU, offset=1, preview=False)
    add("constraint schedule None", eng.set_constraint_schedule, 0, None, NU)
    add("constraint schedule: wrong r", eng.set_constraint_schedule, 0, A(6, NU + 1), NU)
    add("constraint schedule: 4-d", eng.set_constraint_schedule, 0, A(1, b, 6, NU), NU)
    add("bound schedule", eng.set_control_bound_schedule, -np.abs(A(6, NU)), np.abs(A(6, NU)))
    add("bound schedule per instance, offset, no preview", eng.set_control_bound_schedule, -np.abs(A(b, 5, NU)), np.abs(A(b, 5, NU)), offset=2,
        preview=False)
    add("bound schedule None", eng.set_control_bound_schedule, None, None)
    add("bound schedule: one of two", eng.set_control_bound_schedule, A(6, NU), None)
    add("bound schedule: once and per instance", eng.set_control_bound_schedule, A(6, NU), A(b, 6, NU))
    add("bound schedule: steps differ", eng.set_control_bound_schedule, A(6, NU), A(7, NU))
    add("bound schedule: wrong r", eng.set_control_bound_schedule, A(6, NU + 1), A(6, NU + 1))
    # the weight rule
    add("bias gain diagonal", eng.set_bias_estimator, A(NX))
    add("bias gain dense", eng.set_bias_estimator, A(NX, NX))
    add("bias gain diagonal per instance", eng.set_bias_estimator, A(b, NX))
    add("bias gain dense per instance", eng.set_bias_estimator, A(b, NX, NX))
    add("bias gain None", eng.set_bias_estimator, None)
    add("bias gain: wrong rows", eng.set_bias_estimator, A(NX + 1))
    add("bias gain: wrong batch", eng.set_bias_estimator, A(b + 1, NX, NX))
    add("bias", eng.set_bias, A(b, NX))
    add("bias: wrong shape", eng.set_bias, A(b, NX + 1))
    add("plant state", eng.set_plant_state, A(b, NX))
    add("plant state: wrong shape", eng.set_plant_state, A(NX))
    # the observer: matrices in natural indexing
    add("noise with the observer off", eng.set_noise, 3, process=np.abs(A(NX)), sensor=np.abs(A(NY)))
    add("tick: the observer's arguments while it is off", eng.advance, noise=np.ones((b, NY)))
    add("rollout: the observer's histories while it is off", eng.rollout, 2, y_hist=True)
    add("observer", eng.set_observer, A(NY, NX), A(NX, NY))
    add("observer with Ld", eng.set_observer, A(NY, NX), A(NX, NY), A(NX, NY))
    add("observer per instance", eng.set_observer, A(b, NY, NX), A(b, NX, NY), A(b, NX, NY))
    add("observer: C per instance, gains once", eng.set_observer, A(b, NY, NX), A(NX, NY), A(NX, NY))
    add("observer: Ld per instance, the rest once", eng.set_observer, A(NY, NX), A(NX, NY), A(b, NX, NY))
    add("observer: no Lx", eng.set_observer, A(NY, NX))
    add("observer: Lx not transposed", eng.set_observer, A(NY, NX), A(NY, NX))
    add("observer: C 1-d", eng.set_observer, A(NX), A(NX, NY))
    add("observer: wrong batch", eng.set_observer, A(b + 1, NY, NX), A(b + 1, NX, NY))
    add("noise once", eng.set_noise, 7, process=np.abs(A(NX)), sensor=np.abs(A(NY)))
    add("noise per instance, first instance", eng.set_noise, 2 ** 40 + 1, process=np.abs(A(b, NX)), sensor=np.abs(A(b, NY)), first_instance=11)
    add("noise process only", eng.set_noise, 1, process=np.abs(A(NX)))
    add("noise sensor only", eng.set_noise, 1, sensor=np.abs(A(b, NY)))
    add("noise None", eng.set_noise, 1)
    add("noise: once and per instance", eng.set_noise, 1, process=A(NX), sensor=A(b, NY))
    add("noise: wrong rows", eng.set_noise, 1, process=A(NX + 1))
    add("noise: sensor wrong rows", eng.set_noise, 1, sensor=A(NY + 1))
    add("draw noise: no such stream", eng.draw_noise, 0, stream="both")
    add("observer None", eng.set_observer, None)
    # the score: both rules, and the two write-outs
    add("score diagonal", eng.set_score, np.abs(A(NX)), np.abs(A(NU)))
    add("score dense", eng.set_score, A(NX, NX), A(NU, NU), tol=0.5)
    add("score: dense beside diagonal", eng.set_score, A(NX, NX), np.abs(A(NU)))
    add("score: diagonal beside dense", eng.set_score, np.abs(A(NX)), A(NU, NU))
    add("score diagonal per instance", eng.set_score, np.abs(A(b, NX)), np.abs(A(b, NU)))
    add("score dense per instance", eng.set_score, A(b, NX, NX), A(b, NU, NU))
    add("score: dense per instance beside diagonal once", eng.set_score, A(b, NX, NX), np.abs(A(NU)))
    add("score: diagonal per instance beside dense once", eng.set_score, np.abs(A(b, NX)), A(NU, NU))
    add("score constant goal", eng.set_score, np.abs(A(NX)), state_ref=A(NX))
    add("score signal", eng.set_score, np.abs(A(NX)), state_ref=A(7, NX))
    add("score signal of batch steps", eng.set_score, np.abs(A(NX)), state_ref=A(b, NX))
    add("score signal per instance", eng.set_score, np.abs(A(NX)), state_ref=A(b, 7, NX))
    add("score signal per instance beside weights per instance", eng.set_score, np.abs(A(b, NX)), np.abs(A(b, NU)), state_ref=A(b, 3, NX))
    add("score constant goal beside per-instance weights", eng.set_score, np.abs(A(b, NX)), state_ref=A(NX))
    add("score limits", eng.set_score, state_limits=(-np.abs(A(NX)), np.abs(A(NX))), control_limits=(-np.abs(A(NU)), np.abs(A(NU))))
    add("score limits per instance", eng.set_score, state_limits=(-np.abs(A(b, NX)), np.abs(A(b, NX))),
        control_limits=(-np.abs(A(b, NU)), np.abs(A(b, NU))), tol=1e-3)
    add("score: limits once and per instance, infinite entries", eng.set_score, np.abs(A(NX)), state_limits=(np.full(NX, -np.inf), np.abs(A(b, NX))),
        control_limits=(-np.abs(A(b, NU)), np.full(NU, np.inf)))
    add("score everything", eng.set_score, A(NX, NX), np.abs(A(b, NU)), A(5, NX), (-np.abs(A(NX)), np.abs(A(b, NX))), (-np.abs(A(NU)), np.abs(A(NU))), 0.25)
    add("score None", eng.set_score, None)
    add("score: wrong weight rows", eng.set_score, A(NX + 1))
    add("score: 3-d control weights of the wrong batch", eng.set_score, None, A(b + 1, NU, NU))
    add("score: wrong goal", eng.set_score, A(NX), state_ref=A(NX + 1))
    add("score: wrong signal batch", eng.set_score, A(NX), state_ref=A(b + 1, 3, NX))
    add("score: dense limits", eng.set_score, A(NX), state_limits=(A(NX + 1, NX + 1), A(NX)))
    # the targets
    add("target constant", eng.set_target, A(NU, NX), A(NU), costs=[0])
    add("target signal, offset, two costs", eng.set_target, A(NU, NX), A(6, NU), costs=[2, 0], offset=2)
    add("target signal of batch steps", eng.set_target, A(NU, NX), A(b, NU), costs=[1])
    add("target signal per instance", eng.set_target, A(NU, NX), A(b, 6, NU), costs=(0, 1, 2))
    add("target None", eng.set_target, None)
    add("target: no setpoint", eng.set_target, A(NU, NX), None, costs=[0])
    add("target: no costs", eng.set_target, A(NU, NX), A(NU), costs=[])
    add("target: no such cost", eng.set_target, A(NU, NX), A(NU), costs=[3])
    add("target: outputs not (nu, nx)", eng.set_target, A(NX, NU), A(NU), costs=[0])
    add("target: outputs 1-d", eng.set_target, A(NX), A(NU), costs=[0])
    add("target: wrong setpoint", eng.set_target, A(NU, NX), A(NU + 1), costs=[0])
    add("target: wrong setpoint batch", eng.set_target, A(NU, NX), A(b + 1, 6, NU), costs=[0])
    add("target: offset < 0", eng.set_target, A(NU, NX), A(NU), costs=[0], offset=-1)
    # the tick, as far as it goes with nothing on the device
    add("tick", eng.advance)
    add("tick on a stream", eng.advance, stream=12345)
    add("tick: a numpy output", eng.advance, x_out=np.zeros((b, NX)))
    add("rollout", eng.rollout, 3, solve_every=2)
    add("rollout: ticks < 0", eng.rollout, -1)
    add("solve", eng.solve)
    return steps


def run_script(b, monkeypatch=None):
    eng, rec = controller(monkeypatch, b)
    out = [dict(step="create", calls=list(rec.calls))]
    for label, fn in script(eng, b):
        n = len(rec.calls)
        try:
            fn()
            out.append(dict(step=label, calls=rec.calls[n:]))
        except Exception as e:  # (a refusal before the library call: the record is the exception's class)
            out.append(dict(step=label, raises=type(e).__name__, calls=rec.calls[n:]))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("b", BATCHES)
def test_calls_are_the_recorded_ones(b, golden, monkeypatch):
    got = json.loads(json.dumps(run_script(b, monkeypatch)))  # (tuples -> lists, as the file holds them)
    want = golden["batch %d" % b]
    assert [s["step"] for s in got] == [s["step"] for s in want]
    for g, w in zip(got, want):
        assert g == w, g["step"]


def test_script_covers_refusals_and_calls(golden):
    """the golden record is not vacuous: every step either reached the library or was refused before it, and both kinds occur"""
    for steps in golden.values():
        refused = [s for s in steps if "raises" in s]
        assert len(refused) >= 40 and all(c["fn"].endswith("_init") for s in refused for c in s["calls"])  # (a struct's defaults, no more)
        assert all(not s["calls"][-1]["fn"].endswith("_init") for s in steps if "raises" not in s)
        assert {s["raises"] for s in refused} == {"ValueError", "CopraDomainError"}


# ---- B. the device path and the keep-alive slots: CPU tensors stand in for CUDA tensors ----
@pytest.fixture
def resident(monkeypatch):
    """CPU tensors count as resident; what the binding itself copies to the device (set_target's maps) stays where it is"""
    import torch
    from copra_amd import _args
    monkeypatch.setattr(_args, "is_resident", lambda t: True)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda t: t.clone())
    return monkeypatch


def _t(rng, *shape, dtype="float64"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rng.standard_normal(shape).astype(dtype) if dtype != "int32" else np.zeros(shape, dtype=dtype)))


def _observer_on(eng):
    eng.set_observer(np.ones((NY, NX)), np.ones((NX, NY)))


def _np_system(eng, b):
    eng.set_system(np.zeros((b, NX, NX)), np.zeros((b, NX, NU)), np.zeros((b, NX)), np.zeros((b, NX)))


B5 = 5
# name -> dict(fn: the library function of the call; make(rng): [(tensor in ABI layout, its last two axes are a matrix)]; call(eng, *arrays);
#              where: the arguments / struct fields that hold the tensors' pointers, in order; slot: where they are kept (None: nowhere -- copied);
#              ends: {label: a call that ends the slot}, beside the same call with host arrays; prep(eng); twin: numpy goes the same way)
CASES = {
    "set_system": dict(
        fn="copra_batch_set_system", make=lambda g: [(_t(g, B5, NX, NX), 1), (_t(g, B5, NU, NX), 1), (_t(g, B5, NX), 0), (_t(g, B5, NX), 0)],
        call=lambda e, *a: e.set_system(*a), where=("A", "B", "d", "x0"), slot="system", ends={}),
    "set_system_rowmajor_async": dict(
        fn="copra_batch_set_system_rowmajor_async", make=lambda g: [(_t(g, B5, NX, NX), 0), (_t(g, B5, NX, NU), 0), (_t(g, B5, NX), 0), (_t(g, B5, NX), 0)],
        call=lambda e, *a: e.set_system_rowmajor_async(*a), where=("A", "B", "d", "x0"), slot="system", twin=False,
        ends={"set_system from host arrays": lambda e: _np_system(e, B5)}),
    "set_x0": dict(fn="copra_batch_set_x0", make=lambda g: [(_t(g, B5, NX), 0)], call=lambda e, x: e.set_x0(x), where=("x0",), slot="x0", ends={}),
    "set_cost_reference": dict(
        fn="copra_batch_set_cost_reference", make=lambda g: [(_t(g, B5, NX), 0)], call=lambda e, p: e.set_cost_reference(0, p), where=("p",),
        slot=("reference", 0),
        ends={"set_cost_reference(k, None)": lambda e: e.set_cost_reference(0, None),
              "set_cost_reference(k, one for all)": lambda e: e.set_cost_reference(0, np.zeros(NX)),
              "set_reference_schedule(k)": lambda e: e.set_reference_schedule(0, np.zeros((6, NX)), NX),
              "set_target with cost k": lambda e: e.set_target(np.ones((NU, NX)), np.zeros(NU), costs=[1, 0])}),
    "set_cost_weights": dict(
        fn="copra_batch_set_cost_weights", make=lambda g: [(_t(g, B5, NU), 0)], call=lambda e, w: e.set_cost_weights(1, w), where=("w",),
        slot=("weights", 1), ends={"set_cost_weights(k, None)": lambda e: e.set_cost_weights(1, None)}),
    "set_reference_schedule": dict(
        fn="copra_batch_set_reference_schedule", make=lambda g: [(_t(g, B5, 6, NX), 0)], call=lambda e, s: e.set_reference_schedule(0, s, NX, offset=2),
        where=("sched",), slot=("schedule", 0),
        ends={"set_reference_schedule(k, None)": lambda e: e.set_reference_schedule(0, None, NX),
              "set_cost_reference(k, None)": lambda e: e.set_cost_reference(0, None),
              "set_cost_reference(k, p)": lambda e: e.set_cost_reference(0, np.zeros((B5, NX)))}),
    "set_constraint_schedule": dict(
        fn="copra_batch_set_constraint_schedule", make=lambda g: [(_t(g, 6, NU), 0)],
        call=lambda e, s: e.set_constraint_schedule(0, s, NU, offset=1, preview=False), where=("sched",), slot=("limit", 0),
        ends={"set_constraint_schedule(k, None)": lambda e: e.set_constraint_schedule(0, None, NU),
              "set_constraint_rhs(k)": lambda e: e.set_constraint_rhs(0, np.zeros((B5, NU)))}),
    "set_control_bound_schedule": dict(
        fn="copra_batch_set_control_bound_schedule", make=lambda g: [(_t(g, B5, 6, NU), 0), (_t(g, B5, 6, NU), 0)],
        call=lambda e, lo, up: e.set_control_bound_schedule(lo, up), where=("lower", "upper"), slot=("limit", "bounds"),
        ends={"set_control_bound_schedule(None, None)": lambda e: e.set_control_bound_schedule(None, None),
              "set_control_bounds": lambda e: e.set_control_bounds(-1.0, 1.0)}),
    "set_bias_estimator": dict(
        fn="copra_batch_set_bias_estimator", make=lambda g: [(_t(g, B5, NX, NX), 1)], call=lambda e, L: e.set_bias_estimator(L), where=("gain",),
        slot="bias", ends={"set_bias_estimator(None)": lambda e: e.set_bias_estimator(None)}),
    "set_bias": dict(fn="copra_batch_set_bias", make=lambda g: [(_t(g, B5, NX), 0)], call=lambda e, d: e.set_bias(d), where=("d",), slot=None),
    "set_plant_state": dict(fn="copra_batch_set_plant_state", make=lambda g: [(_t(g, B5, NX), 0)], call=lambda e, x: e.set_plant_state(x),
                            where=("x",), slot=None),
    "set_cost_reference for all": dict(fn="copra_batch_set_cost_reference_all", make=lambda g: [(_t(g, NX), 0)],
                                       call=lambda e, p: e.set_cost_reference(0, p), where=("p",), slot=None),
    "set_observer": dict(
        fn="copra_batch_set_observer", make=lambda g: [(_t(g, B5, NX, NY), 1), (_t(g, B5, NY, NX), 1), (_t(g, B5, NY, NX), 1)],
        call=lambda e, *a: e.set_observer(*a), where=("C", "Lx", "Ld"), slot="observer",
        ends={"set_observer(None)": lambda e: e.set_observer(None), "set_shared_system": lambda e: e.set_shared_system(np.eye(NX), np.ones((NX, NU)), np.zeros(NX))}),
    "set_noise": dict(
        fn="copra_batch_set_noise", prep=_observer_on, make=lambda g: [(_t(g, B5, NX), 0), (_t(g, B5, NY), 0)],
        call=lambda e, w, v: e.set_noise(9, process=w, sensor=v, first_instance=3), where=("sigma_w", "sigma_v"), slot="noise",
        ends={"set_noise(seed)": lambda e: e.set_noise(9)}),
    "draw_noise": dict(fn="copra_batch_draw_noise", make=lambda g: [(_t(g, B5, NX), 0)], call=lambda e, out: [e.draw_noise(4, out=out)] and None,
                       where=("out_device",), slot=None, twin=False),
    "set_score": dict(
        fn="copra_batch_set_score",
        make=lambda g: [(_t(g, B5, NX, NX), 1), (_t(g, B5, NU, NU), 1), (_t(g, B5, 3, NX), 0)] + [(_t(g, B5, r), 0) for r in (NX, NX, NU, NU)],
        call=lambda e, qx, ru, ref, xl, xh, ul, uh: e.set_score(qx, ru, ref, (xl, xh), (ul, uh), 0.5),
        where=("qx", "ru", "x_ref", "x_lo", "x_hi", "u_lo", "u_hi"), slot="score", ends={"set_score(None)": lambda e: e.set_score(None)}),
    "set_target": dict(
        fn="copra_batch_set_target", make=lambda g: [(_t(g, NX, NU), 1), (_t(g, B5, 6, NU), 0)],
        call=lambda e, H, r: e.set_target(H, r, costs=[2, 0], offset=1), where=("H", "r"), slot="target",
        ends={"set_target(None)": lambda e: e.set_target(None), "set_shared_system": lambda e: e.set_shared_system(np.eye(NX), np.ones((NX, NU)), np.zeros(NX))}),
    "advance": dict(
        fn="copra_batch_advance", prep=_observer_on, twin=False,
        make=lambda g: [(_t(g, B5, NX, NX), 0), (_t(g, B5, NU, NX), 0), (_t(g, B5, NX), 0), (_t(g, B5, NX), 0), (_t(g, B5, NU), 0), (_t(g, B5, NX), 0),
                        (_t(g, B5, dtype="int32"), 0), (_t(g, B5, NY), 0), (_t(g, B5, NY), 0)],
        call=lambda e, A, B, d, w, fu, xo, so, v, yo: e.advance(plant=(A, B, d), disturbance=w, fallback_control=fu, x_out=xo, status_out=so, noise=v,
                                                                y_out=yo),
        where=("A", "B", "d", "w", "fallback_u", "x_out", "status_out", "v", "y_out"), slot="tick", ends={"the next tick": lambda e: e.advance()}),
    "rollout": dict(
        fn="copra_batch_rollout", twin=False,
        make=lambda g: [(_t(g, 3, B5, NX), 0), (_t(g, 4, B5, NX), 0), (_t(g, 3, B5, dtype="int32"), 0), (_t(g, 3, B5, NX), 0), (_t(g, B5, NU), 0)],
        call=lambda e, ws, xh, ah, dh, uo: e.rollout(3, disturbances=ws, x_hist=xh, age_hist=ah, d_hist=dh, u_out=uo),
        where=("w_seq", "x_hist", "age_hist", "d_hist", "u_out"), slot="tick", ends={"the next tick": lambda e: e.rollout(1)}),
}


def _without_residency(entry):
    return {k: (_without_residency(v) if isinstance(v, dict) else v) for k, v in entry.items() if k != "on_device"}


def _fresh(case, resident, seed=7):
    eng, rec = controller(resident, B5)
    case.get("prep", lambda e: None)(eng)
    made = case["make"](np.random.default_rng(seed))
    return eng, rec, [t for t, _ in made], [bool(m) for _, m in made]


@pytest.mark.parametrize("name", sorted(CASES))
def test_tensors_are_used_in_place_with_the_flags_of_numpy(name, resident):
    case = CASES[name]
    eng, rec, tensors, matrix = _fresh(case, resident)
    case["call"](eng, *tensors)
    call, raw = rec.calls[-1], rec.raw[-1]
    assert call["fn"] == case["fn"]
    assert [raw[w] for w in case["where"]] == [t.data_ptr() for t in tensors]
    structs = [v for v in call.values() if isinstance(v, dict)]
    if "on_device" in call or (structs and "on_device" in structs[0]):  # (the tick's arrays are device pointers by contract: no flag)
        assert (call if "on_device" in call else structs[0])["on_device"] == 1
    if case.get("twin", True):  # the equivalent numpy call: natural indexing, so a matrix is the tensor's transpose
        twin, trec, _, _ = _fresh(case, resident)
        case["call"](twin, *[np.swapaxes(t.numpy(), -1, -2) if m else t.numpy() for t, m in zip(tensors, matrix)])
        host = trec.calls[-1]
        assert (host if "on_device" in host else [v for v in host.values() if isinstance(v, dict)][0])["on_device"] == 0
        assert _without_residency(host) == _without_residency(call)  # per_instance, dense, steps, offsets -- and the bytes


def _alive(refs):
    gc.collect()
    return [r() is not None for r in refs]


@pytest.mark.parametrize("name", sorted(CASES))
def test_slot_holds_until_its_table_says(name, resident):
    case = CASES[name]
    eng, rec, tensors, matrix = _fresh(case, resident)
    case["call"](eng, *tensors)
    refs = [weakref.ref(t) for t in tensors]
    hosts = [np.swapaxes(t.numpy(), -1, -2).copy() if m else t.numpy().copy() for t, m in zip(tensors, matrix)]
    del tensors
    if case["slot"] is None:  # copied by the library before it returns: nothing is kept
        assert _alive(refs) == [False] * len(refs)
        return
    assert case["slot"] in eng._held and all(_alive(refs)), "kept while the library reads them"
    # a replacing call that the library refuses leaves the tensors in force where they are
    rec.refuse.add(case["fn"])
    with pytest.raises(ValueError):
        case["call"](eng, *_fresh(case, resident, seed=8)[2])
    rec.refuse.clear()
    assert all(_alive(refs)), "a refused call released the tensors the library still reads"
    # an accepted one takes their place
    other = _fresh(case, resident, seed=9)[2]
    case["call"](eng, *other)
    assert not any(_alive(refs)), "replaced, and still held"
    # every call of the table that ends the slot, one by one
    ends = dict(case["ends"])
    if case.get("twin", True):
        ends["the same call from host arrays"] = lambda e: case["call"](e, *hosts)
    for label, end in ends.items():
        eng, rec, tensors, _ = _fresh(case, resident)
        case["call"](eng, *tensors)
        refs = [weakref.ref(t) for t in tensors]
        del tensors
        assert all(_alive(refs))
        end(eng)
        assert case["slot"] not in eng._held and not any(_alive(refs)), label


def test_other_slots_are_left_alone(resident):
    """ending one slot ends no other: every family set from tensors, then one call after the other of the release table"""
    eng, rec = controller(resident, B5)
    rng = np.random.default_rng(3)
    made = {}
    for name in ("set_system", "set_x0", "set_cost_weights", "set_constraint_schedule", "set_control_bound_schedule", "set_bias_estimator",
                 "set_observer", "set_noise", "set_score", "set_reference_schedule"):
        made[name] = [t for t, _ in CASES[name]["make"](rng)]
        CASES[name]["call"](eng, *made[name])
    slots = {CASES[n]["slot"] for n in made}
    assert set(eng._held) == slots
    for end, slot in ((lambda: eng.set_cost_reference(0, None), ("schedule", 0)), (lambda: eng.set_constraint_rhs(0, np.zeros((B5, NU))), ("limit", 0)),
                      (lambda: eng.set_control_bounds(-1, 1), ("limit", "bounds")), (lambda: eng.set_cost_weights(1, None), ("weights", 1)),
                      (lambda: eng.set_shared_system(np.eye(NX), np.ones((NX, NU)), np.zeros(NX)), "observer"),
                      (lambda: eng.set_noise(1), "noise"), (lambda: eng.set_score(None), "score"), (lambda: eng.set_bias_estimator(None), "bias")):
        end()
        slots.discard(slot)
        assert set(eng._held) == slots, slot
    assert slots == {"system", "x0"}


def test_outputs_are_held(resident):
    eng, rec = controller(resident, B5)
    outs = [_t(np.random.default_rng(0), B5, n) for n in (NU * N, NX * (N + 1))] + [_t(None, B5, dtype="int32"), _t(None, B5, 2, dtype="int32")]
    eng.set_outputs(*outs)
    assert [rec.raw[-1][k] for k in ("control", "trajectory", "status", "iter")] == [t.data_ptr() for t in outs]
    refs = [weakref.ref(t) for t in outs]
    del outs
    assert all(_alive(refs))


# the refusals that the binding makes before the library could read a pointer it must not: (entry point, the call with tensor t)
TENSOR_ENTRIES = {"set_x0": ((B5, NX), lambda e, t: e.set_x0(t)),
                  "set_cost_reference": ((B5, NX), lambda e, t: e.set_cost_reference(0, t)),
                  "set_cost_reference for all": ((NX,), lambda e, t: e.set_cost_reference(0, t))}


def _bad_tensors(shape):
    """name -> (a tensor, the exception it earns where CPU tensors count as resident)"""
    import torch
    wide = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=torch.float64)
    assert not wide[..., ::2].is_contiguous() and tuple(wide[..., ::2].shape) == tuple(shape)
    return {"float32": (torch.zeros(shape, dtype=torch.float32), ValueError),
            "not contiguous": (wide[..., ::2], ValueError),
            "wrong shape": (torch.zeros(shape[:-1] + (shape[-1] + 1,), dtype=torch.float64), _capi.CopraDomainError)}


@pytest.mark.parametrize("entry", sorted(TENSOR_ENTRIES))
def test_tensors_that_were_passed_on_unchecked_are_refused(entry, monkeypatch):
    import torch
    shape, call = TENSOR_ENTRIES[entry]
    eng, rec = controller(monkeypatch, B5)
    n = len(rec.calls)
    bad = dict(_bad_tensors(shape), **{"on the host": (torch.zeros(shape, dtype=torch.float64), ValueError)})
    for what, (t, _) in bad.items():  # the residency test as shipped: none of them is on the device
        with pytest.raises(ValueError):
            call(eng, t)
    assert rec.calls[n:] == [] and not eng._held, "the library saw a refused tensor"


@pytest.mark.parametrize("entry", sorted(TENSOR_ENTRIES))
def test_resident_tensors_are_refused_for_their_own_fault(entry, resident):
    shape, call = TENSOR_ENTRIES[entry]
    eng, rec = controller(resident, B5)
    n = len(rec.calls)
    for what, (t, exc) in _bad_tensors(shape).items():
        with pytest.raises(exc):
            call(eng, t)
        if exc is ValueError:
            with pytest.raises(ValueError) as info:
                call(eng, t)
            assert not isinstance(info.value, _capi.CopraDomainError), what
    assert rec.calls[n:] == [] and not eng._held


def test_host_arrays_that_were_passed_on_unchecked_are_refused(monkeypatch):
    eng, rec = controller(monkeypatch, B5)
    n = len(rec.calls)
    for call in (lambda: eng.set_x0(np.zeros((B5, NX + 1))), lambda: eng.set_x0(np.zeros(NX)), lambda: eng.set_x0(np.zeros((B5 + 1, NX))),
                 lambda: eng.set_constraint_rhs(0, np.zeros((B5 + 1, NU))), lambda: eng.set_constraint_rhs(0, np.zeros(())),
                 lambda: eng.set_cost_reference(0, np.zeros((B5 + 1, NX)))):
        with pytest.raises(_capi.CopraDomainError):
            call()
    assert rec.calls[n:] == []


def test_what_were_asserts_are_exceptions(resident, monkeypatch):
    """set_system, set_system_rowmajor_async, set_cost_weights: the checks survive python -O"""
    import torch
    from copra_amd import _args
    eng, rec = controller(resident, B5)
    n = len(rec.calls)
    good = [np.zeros((B5, NX, NX)), np.zeros((B5, NX, NU)), np.zeros((B5, NX)), np.zeros((B5, NX))]
    for i, wrong in enumerate((np.zeros((B5, NX, NX + 1)), np.zeros((B5, NU, NX)), np.zeros((B5 + 1, NX)), np.zeros(NX))):
        with pytest.raises(_capi.CopraDomainError):
            eng.set_system(*[wrong if j == i else a for j, a in enumerate(good)])
    with pytest.raises(ValueError):  # (host arrays: this entry point takes tensors only)
        eng.set_system_rowmajor_async(*good)
    with pytest.raises(ValueError):  # a tensor among arrays
        eng.set_system(torch.zeros(B5, NX, NX, dtype=torch.float64), *good[1:])
    monkeypatch.setattr(_args, "is_resident", lambda t: t.is_cuda)
    tensors = [torch.zeros(a.shape, dtype=torch.float64) for a in good]
    for call in (lambda: eng.set_system(*tensors), lambda: eng.set_system_rowmajor_async(*tensors),
                 lambda: eng.set_cost_weights(1, torch.zeros(B5, NU, dtype=torch.float64)),
                 lambda: eng.set_cost_weights(1, torch.zeros(NU, dtype=torch.float64))):
        with pytest.raises(ValueError):
            call()
    assert rec.calls[n:] == [] and not eng._held


# ---- C. the two shape rules ----
@pytest.mark.parametrize("r,b", [(4, 5), (4, 4), (2, 5), (1, 3), (3, 1)])
def test_weight_rule(r, b):
    from copra_amd._args import weight_form
    assert weight_form((r,), r, b) == (0, 0)
    assert weight_form((r, r), r, b) == (1, 0)
    assert weight_form((b, r), r, b) == ((1, 0) if b == r else (0, 1))  # the tie: a 2-d array is read as (r, r)
    assert weight_form((b, r, r), r, b) == (1, 1)
    assert weight_form([b, r, r], r, b) == (1, 1)
    for shape in ((), (r + 1,), (b, r + 1), (b + 1, r) if b + 1 != r else (b + 2, r), (r, r + 1), (b + 1, r, r), (b, r, r + 1), (b, r + 1, r), (1, b, r, r)):
        with pytest.raises(_capi.CopraDomainError):
            weight_form(shape, r, b, "w")
    # a vector of r rows: no dense form, so no tie either
    assert weight_form((r,), r, b, dense_allowed=False) == (0, 0)
    assert weight_form((b, r), r, b, dense_allowed=False) == (0, 1)
    for shape in ((r, r), (b, r, r), (r + 1,), ()):
        if shape != (b, r):
            with pytest.raises(_capi.CopraDomainError):
                weight_form(shape, r, b, "w", dense_allowed=False)


@pytest.mark.parametrize("r,b", [(4, 5), (4, 4), (2, 5), (5, 2)])
def test_signal_rule(r, b):
    from copra_amd._args import signal_form
    assert signal_form((r,), r, b, True) == (1, 0)
    assert signal_form((7, r), r, b, True) == signal_form((7, r), r, b, False) == (7, 0)
    assert signal_form((1, r), r, b, False) == (1, 0)
    assert signal_form((b, r), r, b, False) == (b, 0)  # steps == batch: a 2-d signal is ONE signal of `batch` steps
    assert signal_form((r, r), r, b, True) == (r, 0)
    assert signal_form((b, 7, r), r, b, False) == (7, 1)
    assert signal_form((b, b, r), r, b, True) == (b, 1)
    assert signal_form((b, 1, r), r, b, True) == (1, 1)
    for shape, constant in (((r,), False), ((), True), ((r + 1,), True), ((0, r), True), ((7, r + 1), False), ((b, 0, r), False), ((b + 1, 7, r), True),
                            ((b, 7, r + 1), True), ((1, b, 7, r), True)):
        with pytest.raises(_capi.CopraDomainError):
            signal_form(shape, r, b, constant, "s")


# ---- D. on the device: a refused call changes nothing ----
def _planar(b):
    """a CoM double integrator in the plane (nx 4, nu 2), horizon 3, per-instance sampling periods, a control bound that binds"""
    T = np.linspace(0.08, 0.15, b)
    A, B = np.tile(np.eye(NX), (b, 1, 1)), np.zeros((b, NX, NU))
    A[:, :2, 2:] = T[:, None, None] * np.eye(2)
    B[:, :2] = (0.5 * T * T)[:, None, None] * np.eye(2)
    B[:, 2:] = T[:, None, None] * np.eye(2)
    x0 = np.array([1.5, 0.3, 0.0, 0.0]) + 0.05 * np.arange(b * NX).reshape(b, NX) / (b * NX)
    costs = [dict(kind="trajectory", M=np.eye(NX), p=np.array([1.6, 0.4, 0.05, 0.3]), weights=[10.0, 10.0, 1.0, 1.0]),
             dict(kind="control", N=np.eye(NU), p=np.zeros(NU), weights=[1e-3] * NU)]
    cstrs = [dict(kind="control", G=np.eye(NU), f=np.full(NU, 2.5)), dict(kind="control_bound", lower=[-1.2] * NU, upper=[1.2] * NU)]
    return dict(A=A, B=B, d=np.zeros((b, NX)), x0=x0, costs=costs, cstrs=cstrs)


@pytest.mark.gpu
def test_refused_tensors_leave_the_controller_as_its_twin():
    import torch
    wl = _planar(B5)
    goals = wl["costs"][0]["p"] + 0.01 * np.arange(B5 * NX).reshape(B5, NX)
    engines = []
    for _ in range(2):
        eng = batch_mod.BatchLMPC(NX, NU, N, B5, wl["costs"], wl["cstrs"])
        eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
        eng.goals = torch.from_numpy(goals).cuda()
        eng.set_cost_reference(0, eng.goals)
        engines.append(eng)
    eng, never = engines

    def cuda(shape, dtype=torch.float64):
        return torch.ones(shape, dtype=dtype, device="cuda")

    refused = [(lambda: eng.set_x0(cuda((B5, NX), torch.float32)), ValueError), (lambda: eng.set_x0(cuda((B5, NX + 1))), _capi.CopraDomainError),
               (lambda: eng.set_x0(cuda((B5, 2 * NX))[:, ::2]), ValueError), (lambda: eng.set_x0(cuda((NX,))), _capi.CopraDomainError),
               (lambda: eng.set_x0(np.ones((B5, NX + 1))), _capi.CopraDomainError),
               (lambda: eng.set_cost_reference(0, cuda((B5, NX), torch.float32)), ValueError),
               (lambda: eng.set_cost_reference(0, cuda((B5, NX - 1))), _capi.CopraDomainError),
               (lambda: eng.set_cost_reference(0, cuda((B5 + 1, NX))), _capi.CopraDomainError),
               (lambda: eng.set_cost_reference(0, cuda((2 * NX,))[::2]), ValueError),
               (lambda: eng.set_cost_reference(0, cuda((NX,), torch.float32)), ValueError),
               (lambda: eng.set_cost_reference(0, cuda((NX + 1,))), _capi.CopraDomainError),
               (lambda: eng.set_cost_reference(0, torch.ones(B5, NX, dtype=torch.float64)), ValueError),
               (lambda: eng.set_constraint_rhs(0, np.ones((B5 + 1, NU))), _capi.CopraDomainError)]
    for call, exc in refused:
        with pytest.raises(exc):
            call()
    assert eng._held[("reference", 0)] is eng.goals and "x0" not in eng._held
    res = []
    for e in engines:
        e.solve()
        res.append(e.results())
    assert (res[0]["status"] == 0).all()
    assert np.abs(res[0]["control"]).max() > 1.0  # (the problem is not a trivial one: controls near their bound)
    for k in ("control", "trajectory", "status", "iter"):
        assert np.array_equal(res[0][k], res[1][k]), k


if __name__ == "__main__":
    record = {"batch %d" % b: run_script(b) for b in BATCHES}
    with open(GOLDEN, "w") as fh:
        json.dump(record, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("%s: %d bytes, %s steps" % (GOLDEN, os.path.getsize(GOLDEN), [len(v) for v in record.values()]))
