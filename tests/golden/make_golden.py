"""Generate golden fixtures from the reference (runs ONLY in the build container).

The reference package cannot be imported as a whole here (casadi / pyproprop are not
installed).  Two of its numeric modules do load by file path:

* ``pycollo/mesh.py``        -- needs numpy/scipy only.
* ``pycollo/quadrature.py``  -- needs ``pyproprop.Options`` at import time, used for one
  module-level constant (``QUADRATURES``, quadrature.py:34-35).  A 10-line container class
  with no arithmetic is placed in ``sys.modules`` for that single name; every
  number written below is computed by the reference's own code.

Also copies the *data arrays* of the reference's unit-test data modules
(tests/unit/iteration_scaling_test_data_{brachistochrone,double_pendulum}.py, numpy only).

``pycollo/mesh_refinement.py`` loads under a synthetic ``pycollo`` package object whose ``__path__`` is the
reference (its relative imports then resolve to the reference's own files), with inert stand-ins for ``casadi`` and
``pyproprop``; its ``next_iteration_phase_mesh`` -- plain NumPy / SciPy -- is called unbound on a namespace that carries
the settings, the mesh and the errors, and ``PhaseMesh`` is replaced by a recorder of its keyword arguments.

Outputs (committed): tests/golden/quadrature_tables.npz, mesh_tables.npz, known_answers.npz, next_mesh_cases.npz
The reference never travels to the GPU box; only these .npz files do.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Options:  # stand-in for pyproprop.Options: a bag of names, no arithmetic
    def __init__(self, options, default=None, unsupported=None, handles=None):
        self.options = tuple(options)
        self.default = default
        self.unsupported = unsupported
        self.handles = handles


class _Inert(types.ModuleType):  # stand-in for casadi: any attribute is a name that is never called here
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def _next_mesh_cases():
    """About 300 seeded inputs of the reference's next-mesh rule: K in 1..30, orders within (4, 10) or (2, 20),
    tolerances 1e-7 / 1e-5, errors log-uniform in 1e-17..1, plus forced structure."""
    rng = np.random.default_rng(20240607)
    cases = []

    def add(nodes, h, err, tol, n_min, n_max, tag):
        cases.append(dict(nodes=np.asarray(nodes, np.int64), h=np.asarray(h, float), err=np.asarray(err, float), tol=tol,
                          n_min=n_min, n_max=n_max, tag=tag))
    for i in range(264):
        K = int(rng.integers(1, 31))
        n_min, n_max = ((4, 10), (2, 20))[i % 2]
        tol = (1e-7, 1e-5)[(i // 2) % 2]
        nodes = rng.integers(n_min, n_max + 1, K)
        h = rng.uniform(0.2, 1.0, K)
        h = 2.0 * h / h.sum()
        add(nodes, h, 10.0 ** rng.uniform(-17, 0, K), tol, n_min, n_max, "random")
    for i in range(36):
        K = int(rng.integers(8, 31))
        n_min, n_max = ((4, 10), (2, 20))[i % 2]
        tol = (1e-7, 1e-5)[(i // 2) % 2]
        nodes = rng.integers(n_min, n_max + 1, K)
        h = rng.uniform(0.2, 1.0, K)
        h = 2.0 * h / h.sum()
        err = 10.0 ** rng.uniform(np.log10(tol) - 1, 0, K)       # around and above the tolerance
        kind = ("run_start", "run_middle", "run_end", "run_long", "equal_tol", "zero", "all_below", "zero_only",
                "equal_tol_only")[i % 9]
        over = lambda m: tol * 10.0 ** rng.uniform(-10, -8, m)   # resolved far better than asked: merge candidates
        if kind == "run_start":
            err[:3] = over(3)
        elif kind == "run_middle":
            err[K // 2 - 1:K // 2 + 2] = over(3)
        elif kind == "run_end":
            err[-3:] = over(3)
        elif kind == "run_long":                                  # many narrow high-order sections: >= 3 merged ones
            err[1:8] = over(7)
            nodes[1:8] = n_max
        elif kind == "equal_tol":
            err[K // 3] = tol
        elif kind == "zero":
            err[K // 3] = 0.0
        elif kind == "all_below":
            err = tol * 10.0 ** rng.uniform(-6, -0.01, K)
        elif kind == "zero_only":
            err = np.zeros(K)
        elif kind == "equal_tol_only":
            err = np.full(K, tol)
        add(nodes, h, err, tol, n_min, n_max, kind)
    return cases


def _record_next_mesh():
    import importlib
    import warnings
    pkg = types.ModuleType("pycollo")
    pkg.__path__ = [f"{REF}/pycollo"]
    sys.modules["pycollo"] = pkg
    sys.modules.setdefault("casadi", _Inert("casadi"))
    ref = importlib.import_module("pycollo.mesh_refinement")
    recorded = {}
    ref.PhaseMesh = lambda **kw: recorded.update(kw) or "recorded"   # keeps its keyword arguments, computes nothing
    fn = ref.PattersonRaoMeshRefinement.next_iteration_phase_mesh
    out = {}
    cases = _next_mesh_cases()
    tags, rows = [], []
    for i, c in enumerate(cases):
        settings = types.SimpleNamespace(mesh_tolerance=c["tol"], collocation_points_min=c["n_min"],
                                         collocation_points_max=c["n_max"])
        phase = types.SimpleNamespace(i=0, ocp_phase=types.SimpleNamespace(mesh="unchanged"))
        me = types.SimpleNamespace(ocp=types.SimpleNamespace(settings=settings),
                                   it=types.SimpleNamespace(mesh=types.SimpleNamespace(N_K=[c["nodes"].copy()], h_K=[c["h"].copy()])),
                                   maximum_relative_mesh_errors=[c["err"].copy()])
        recorded.clear()
        status, sizes, nodes = 0, np.zeros(0), np.zeros(0, np.int64)     # 0: new mesh, 1: mesh kept, 2: raised, 3: non-finite
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                with np.errstate(all="ignore"):
                    got = fn(me, phase)
            if got == "unchanged":
                status = 1
            else:
                sizes = np.asarray(recorded["mesh_section_sizes"], float)
                nodes_f = np.asarray(recorded["number_mesh_section_nodes"], float)
                if not (np.all(np.isfinite(sizes)) and np.all(np.isfinite(nodes_f))):
                    status = 3
                else:
                    nodes = nodes_f.astype(np.int64)
                    assert np.array_equal(nodes, nodes_f) and recorded["number_mesh_sections"] == len(nodes)
        except Exception as exc:  # the reference's own failure is part of the record
            status = 2
            print(f"case {i} ({c['tag']}): the reference raised {type(exc).__name__}: {exc}")
        tags.append(c["tag"])
        rows.append((status, sizes, nodes))
    # flat arrays with offsets (one small file instead of two thousand members)
    cat = lambda parts, dt: np.concatenate([np.asarray(p_, dt).ravel() for p_ in parts]) if parts else np.zeros(0, dt)
    out["in_off"] = np.concatenate([[0], np.cumsum([len(c["nodes"]) for c in cases])]).astype(np.int64)
    out["in_nodes"] = cat([c["nodes"] for c in cases], np.int64)
    out["in_h"] = cat([c["h"] for c in cases], float)
    out["in_err"] = cat([c["err"] for c in cases], float)
    out["in_par"] = np.array([[c["tol"], c["n_min"], c["n_max"]] for c in cases], float)
    out["status"] = np.array([r_[0] for r_ in rows], np.int64)
    out["out_off"] = np.concatenate([[0], np.cumsum([len(r_[2]) for r_ in rows])]).astype(np.int64)
    out["out_sizes"] = cat([r_[1] for r_ in rows], float)
    out["out_nodes"] = cat([r_[2] for r_ in rows], np.int64)
    out["tags"] = np.array(tags)
    np.savez_compressed(f"{HERE}/next_mesh_cases.npz", **out)
    st = out["status"]
    print("next-mesh cases:", len(cases), "new mesh", int(np.sum(st == 0)), "kept", int(np.sum(st == 1)), "raised",
          int(np.sum(st == 2)), "non-finite", int(np.sum(st == 3)))


def main():
    sys.modules.setdefault("pyproprop", types.SimpleNamespace(Options=_Options))
    if "next_mesh" in sys.argv[1:]:      # only (iv): the other fixtures stay as they are
        _record_next_mesh()
        return
    quad_mod = _load("ref_quadrature", f"{REF}/pycollo/quadrature.py")
    mesh_mod = _load("ref_mesh", f"{REF}/pycollo/mesh.py")

    def backend(method, quad=None):
        settings = types.SimpleNamespace(collocation_points_min=2, collocation_points_max=20,
                                         quadrature_method=method)
        b = types.SimpleNamespace(ocp=types.SimpleNamespace(settings=settings))
        b.quadrature = quad
        return b

    # (i) quadrature tables, every order the reference allows (2..20, quadrature.py:36-37), lobatto + radau
    out = {}
    quads = {}
    for method in ("lobatto", "radau"):
        q = quad_mod.Quadrature(backend(method))
        quads[method] = q
        for n in range(2, 21):
            out[f"{method}_{n}_points"] = np.asarray(q.quadrature_point(n), dtype=float)
            out[f"{method}_{n}_weights"] = np.asarray(q.quadrature_weight(n), dtype=float)
            out[f"{method}_{n}_A"] = np.asarray(q.A_matrix(n), dtype=float)
            out[f"{method}_{n}_D"] = np.asarray(q.D_matrix(n), dtype=float)
    np.savez_compressed(f"{HERE}/quadrature_tables.npz", **out)

    # (ii) mesh tables
    cases = {
        "k1n2": ([1.0], [2]),
        "k3n4": ([1 / 3] * 3, [4] * 3),
        "k10n4": ([0.1] * 10, [4] * 10),
        "k10n6": ([0.1] * 10, [6] * 10),
        "ragged": ([0.1, 0.25, 0.05, 0.3, 0.3], [4, 7, 2, 5, 10]),
    }
    mout = {}
    for method in ("lobatto", "radau"):
        b = backend(method, quads[method])
        for name, (sizes, nodes) in cases.items():
            pm = types.SimpleNamespace(mesh_section_sizes=np.array(sizes, dtype=float),
                                       number_mesh_section_nodes=np.array(nodes, dtype=int),
                                       number_mesh_sections=len(nodes))
            m = mesh_mod.Mesh(b, [pm])
            key = f"{method}_{name}"
            mout[f"{key}_sizes"] = np.array(sizes, dtype=float)
            mout[f"{key}_nodes"] = np.array(nodes, dtype=np.int64)
            mout[f"{key}_tau"] = m.tau[0]
            mout[f"{key}_N"] = np.array(m.N[0])
            mout[f"{key}_bounds"] = np.asarray(m.mesh_index_boundaries[0], dtype=np.int64)
            mout[f"{key}_hK"] = m.h_K[0]
            mout[f"{key}_W"] = m.W_matrix[0]
            for nm, mat in (("sI", m.sI_matrix[0]), ("sA", m.sA_matrix[0])):
                mat = mat.tocsr()
                mat.sort_indices()
                mout[f"{key}_{nm}_indptr"] = mat.indptr.astype(np.int64)
                mout[f"{key}_{nm}_indices"] = mat.indices.astype(np.int64)
                mout[f"{key}_{nm}_data"] = mat.data.astype(float)
                mout[f"{key}_{nm}_shape"] = np.array(mat.shape, dtype=np.int64)
    np.savez_compressed(f"{HERE}/mesh_tables.npz", **mout)

    # (iii) unit-test data arrays (tests/unit/iteration_scaling_test_data_*.py)
    kout = {}
    for tag, fname in (("BR", "brachistochrone"), ("DP", "double_pendulum")):
        mod = _load(f"ref_data_{tag}", f"{REF}/tests/unit/iteration_scaling_test_data_{fname}.py")
        for nm in ("V", "R", "V_INV", "X", "X_TILDE"):
            kout[f"EXPECT_{nm}_{tag}"] = np.asarray(getattr(mod, f"EXPECT_{nm}_{tag}"), dtype=float)
    np.savez_compressed(f"{HERE}/known_answers.npz", **kout)

    # (iv) the next-mesh rule: inputs and outputs of the reference's own next_iteration_phase_mesh
    _record_next_mesh()
    print("wrote", sorted(os.listdir(HERE)))


if __name__ == "__main__":
    main()
