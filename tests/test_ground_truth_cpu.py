"""CPU tests of the host layer the native ground-truth evaluators share (ground_truth.py): ``MeasuredBSDF``, ``MeasuredTable`` and
``RoughDielectric`` refuse the same bad arguments in the same words, before any native call, and ``sample_weight`` has one
signature."""
import inspect
import re

import pytest

torch = pytest.importorskip("torch")

from bsdf_diffusion_sampling_amd import ground_truth  # noqa: E402
from bsdf_diffusion_sampling_amd.analytic import RoughDielectric  # noqa: E402
from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF, MeasuredTable  # noqa: E402

N = 8
CLASSES = {"MeasuredBSDF": lambda: MeasuredBSDF.__new__(MeasuredBSDF),      # no file, no handle
           "RoughDielectric": lambda: RoughDielectric(0.3),
           "MeasuredTable": lambda: MeasuredTable([None, None])}            # no native table
POSITIONAL = dict(eval_t=("wi", "wo"), sample_weight=("wi", "wo", "pdf_sa"), sample_t=("wi", "u"), pdf_t=("wi", "wo"))


def _call(obj, method, **changed):
    """``obj.method`` on good CPU arguments of N rows, except for ``changed``."""
    v = torch.zeros(N, 3)
    args = dict(wi=v, wo=v, u=torch.zeros(N, obj.U_COLS), pdf_sa=torch.zeros(N))
    keywords = {k: changed.pop(k) for k in list(changed) if k not in args}
    args.update(changed)
    front = (torch.zeros(N, dtype=torch.int64),) if isinstance(obj, MeasuredTable) else ()
    return getattr(obj, method)(*front, *[args[k] for k in POSITIONAL[method]], **keywords)


@pytest.mark.parametrize("name", list(CLASSES))
def test_every_tensor_call_refuses_the_same_bad_arguments(name, monkeypatch):
    def no_launch(*a):
        raise AssertionError("a native call was reached")
    monkeypatch.setattr(ground_truth, "launch", no_launch)
    obj = CLASSES[name]()
    first = "material_id" if name == "MeasuredTable" else "wi"     # the tensor that fixes N is the first one looked at
    for method in POSITIONAL:
        second = "u" if method == "sample_t" else "wo"
        good = torch.zeros(N, obj.U_COLS if second == "u" else 3)
        rows = [("fp64", {second: good.double()}, second),
                ("5 rows against 8", {second: good[:5]}, second),
                ("CPU tensors", {}, first)]
        if method == "sample_t":
            rows += [("columns of u", {"u": torch.zeros(N, obj.U_COLS + 1)}, "u"),
                     ("out is no triple", {"out": (torch.zeros(N, 3), torch.zeros(N))}, "out")]
        if method != "eval_t":
            rows.append(("length of active", {"active": torch.ones(5, dtype=torch.bool)}, "active"))
            if (name, method) != ("MeasuredBSDF", "sample_weight"):     # which copies any mask across, by design
                rows.append(("float active", {"active": torch.ones(N)}, "active"))
        for what, changed, argument in rows:
            with pytest.raises(ValueError) as e:
                _call(obj, method, **changed)
            msg = str(e.value)
            assert msg.startswith(f"{name}.{method}: ") and re.search(rf"\b{argument}\b", msg), (method, what, msg)


def test_sample_weight_has_one_signature(monkeypatch):
    sigs = {name: inspect.signature(make().sample_weight) for name, make in CLASSES.items()}
    for name, sig in sigs.items():
        kinds = {k: p.kind for k, p in sig.parameters.items()}
        keyword_only = [k for k in kinds if kinds[k] is inspect.Parameter.KEYWORD_ONLY]
        positional = [k for k in kinds if kinds[k] is inspect.Parameter.POSITIONAL_OR_KEYWORD]
        assert keyword_only == ["tint", "firefly_threshold", "active"], name
        assert positional == ["material_id"] * (name == "MeasuredTable") + ["wi", "wo", "pdf_sa"], name
        # None = the class's FIREFLY, which the one body reads when it launches
        assert [sig.parameters[k].default for k in keyword_only] == [None, None, None], name
    assert {n: type(make()).FIREFLY for n, make in CLASSES.items()} == \
        {"MeasuredBSDF": 30.0, "MeasuredTable": 30.0, "RoughDielectric": 3.5}

    # the threshold that reaches the entry point (third argument from the end): the class attribute, read at the call
    launched = []
    monkeypatch.setattr(ground_truth, "check", lambda who, tensors, material_id=None, active=None, coerce_active=False: active)
    monkeypatch.setattr(ground_truth, "launch", lambda entry, device, *a: launched.append(a[-3]))
    for make in CLASSES.values():
        obj = make()
        obj._lead = lambda: None
        _call(obj, "sample_weight")
        monkeypatch.setattr(type(obj), "FIREFLY", 7.25)
        _call(obj, "sample_weight")
        _call(obj, "sample_weight", firefly_threshold=2)
    assert launched == [30.0, 7.25, 2.0, 3.5, 7.25, 2.0, 30.0, 7.25, 2.0]
