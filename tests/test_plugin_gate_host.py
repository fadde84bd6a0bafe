"""CPU: the gate of the reference's plugin seam, replayed without RapidDoc.  The reference accepts a `custom_model` only when
`isinstance(obj, rapid_doc.model.custom.CustomBaseModel)` holds (model_init.py:96-120, batch_analyze.py:359); a stand-in module with an
abstract base of the same shape is put into `sys.modules`, and `rapiddoc_amd.plugin` must open that gate for the three seam models -
and respect the two facts of the reference its docstring names (registry key = class name, `is_seal` in the signature)."""
import inspect
import sys
import types
from abc import ABC, abstractmethod

import pytest


def _stand_in_modules():
    """`rapid_doc`, `rapid_doc.model`, `rapid_doc.model.custom` with a fresh CustomBaseModel: an ABC with one abstract batch_predict"""
    class CustomBaseModel(ABC):
        @abstractmethod
        def batch_predict(self, image_list, **kwargs):
            pass

    mods = {name: types.ModuleType(name) for name in ("rapid_doc", "rapid_doc.model", "rapid_doc.model.custom")}
    mods["rapid_doc"].model = mods["rapid_doc.model"]
    mods["rapid_doc.model"].custom = mods["rapid_doc.model.custom"]
    mods["rapid_doc.model.custom"].CustomBaseModel = CustomBaseModel
    return mods, CustomBaseModel


@pytest.fixture()
def rapid_doc_stand_in(monkeypatch):
    mods, base = _stand_in_modules()
    for name, mod in mods.items():
        monkeypatch.setitem(sys.modules, name, mod)
    return base


def _instances():
    """one instance of every seam class, made without touching the GPU"""
    from rapiddoc_amd import plugin
    return [object.__new__(cls) for cls in plugin.seam_classes()]


def test_the_gate_is_closed_before_and_open_after_registration(rapid_doc_stand_in):
    from rapiddoc_amd import plugin
    base = rapid_doc_stand_in
    objs = _instances()
    assert len(objs) == 3 and not any(isinstance(o, base) for o in objs)                 # what the reference sees today
    assert plugin.register_custom_models() is base
    assert all(isinstance(o, base) for o in objs)
    assert all(issubclass(cls, base) for cls in plugin.seam_classes())
    assert plugin.register_custom_models() is base                                        # idempotent
    assert all(isinstance(o, base) for o in objs)
    assert not isinstance(object(), base) and not isinstance("text", base)               # the gate did not simply fall open


def test_an_explicit_base_needs_no_rapid_doc():
    from rapiddoc_amd import plugin
    assert "rapid_doc" not in sys.modules
    _mods, base = _stand_in_modules()
    assert plugin.register_custom_models(base=base) is base
    assert all(isinstance(o, base) for o in _instances())
    with pytest.raises(TypeError, match="register"):
        plugin.register_custom_models(base=object)


def test_custom_configs_has_exactly_the_keys_asked_for(rapid_doc_stand_in):
    from rapiddoc_amd import plugin
    formula, ocr, table = _instances()
    assert plugin.custom_configs() == {}
    assert plugin.custom_configs(formula=formula) == {"formula_config": {"custom_model": formula}}
    both = plugin.custom_configs(ocr=ocr, table=table)
    assert set(both) == {"ocr_config", "table_config"} and both["ocr_config"]["custom_model"] is ocr and both["table_config"]["custom_model"] is table
    every = plugin.custom_configs(formula, ocr, table)
    assert list(every) == ["formula_config", "ocr_config", "table_config"]
    assert all(set(v) == {"custom_model"} and isinstance(v["custom_model"], rapid_doc_stand_in) for v in every.values())


def test_the_registry_key_of_the_reference_tells_the_three_models_apart(rapid_doc_stand_in):
    """utils/hash_utils.py:33-47 make_hashable: a config's `custom_model` enters the registry key as type(v).__name__"""
    import json

    def make_hashable(value):                                     # the reference's rule, restated for dicts
        return json.dumps({k: type(v).__name__ if k == "custom_model" else v for k, v in value.items()}, sort_keys=True)

    from rapiddoc_amd import plugin
    formula, ocr, table = _instances()
    configs = plugin.custom_configs(formula, ocr, table)
    names = [type(c["custom_model"]).__name__ for c in configs.values()]
    assert names == ["FormulaRecognizer", "RegionTextModel", "Mi355UniTableStructure"] and len(set(names)) == 3
    assert len({make_hashable(c) for c in configs.values()}) == 3
    # the documented limit: a second instance of one class under an otherwise equal config has the same key
    assert make_hashable({"custom_model": ocr}) == make_hashable({"custom_model": _instances()[1]})
    assert "share" in plugin.__doc__ and "registry" in plugin.__doc__


def test_region_text_model_keeps_seal_crops_away_and_takes_batch_size():
    """batch_analyze.py:432-434: seal crops go to a custom OCR model only if its batch_predict names `is_seal`; :313 passes batch_size="""
    from rapiddoc_amd.analyze import RegionTextModel
    sig = inspect.signature(RegionTextModel.batch_predict)
    assert "is_seal" not in sig.parameters
    sig.bind(object(), [], batch_size=16)                          # accepted (TypeError otherwise)
    assert "batch_size" in sig.parameters or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sig.parameters.values())
    from rapiddoc_amd import plugin
    for cls in plugin.seam_classes():
        inspect.signature(cls.batch_predict).bind(object(), [], batch_size=16)


def test_without_rapid_doc_the_error_names_what_is_missing(monkeypatch):
    from rapiddoc_amd import plugin
    monkeypatch.setitem(sys.modules, "rapid_doc", None)            # `import rapid_doc...` raises ImportError
    with pytest.raises(ImportError, match=r"rapid_doc\.model\.custom\.CustomBaseModel"):
        plugin.register_custom_models()
    with pytest.raises(ImportError, match="base="):
        plugin.custom_configs(formula=object())


def test_importing_the_package_does_not_import_rapid_doc():
    import rapiddoc_amd.plugin  # noqa: F401
    assert "rapid_doc" not in sys.modules
