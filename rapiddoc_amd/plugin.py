"""The gate of the reference's plugin seam: an unmodified RapidDoc takes a `formula_config / ocr_config / table_config['custom_model']`
object only when `isinstance(obj, rapid_doc.model.custom.CustomBaseModel)` holds (`atom_model_init`, backend/pipeline/model_init.py:96-120;
`BatchAnalyze._run_table_recognition`, batch_analyze.py:359) - otherwise it SILENTLY builds its own ONNX / torch model.  The engine's three
seam models have the base class's shape (`batch_predict(image_list, **kwargs) -> list[str]`) without subclassing it, because the package
must import without RapidDoc; `register_custom_models` makes them virtual subclasses of the base (an `ABC`) once RapidDoc is there.

    from rapiddoc_amd import plugin
    configs = plugin.custom_configs(formula=FormulaRecognizer(weights, tokenizer_json=..., host_images="stage"),
                                    ocr=RegionTextModel(pipeline, host_images="stage"),
                                    table=Mi355UniTableStructure(...))
    doc_analyze(..., **configs)              # formula_config=..., ocr_config=..., table_config=...

Two facts of the reference that the models respect (tests/test_plugin_gate_host.py replays both):
  * its model registry keys a custom model by `type(v).__name__` (utils/hash_utils.py:33-47), so the three classes carry three different
    names - and two INSTANCES of one class under otherwise equal configs share one registry slot: the reference keeps using the first;
  * `_run_seal_ocr` sends seal crops to a custom OCR model only if `inspect.signature(batch_predict)` has an `is_seal` parameter
    (batch_analyze.py:432-434): `RegionTextModel.batch_predict` does not name it (there is no seal reader here) and takes the `batch_size=`
    keyword the reference passes (batch_analyze.py:277, :313) through `**kwargs`.
"""
from __future__ import annotations

from typing import Optional


def seam_classes() -> tuple:
    """(FormulaRecognizer, RegionTextModel, Mi355UniTableStructure): the classes `register_custom_models` registers"""
    from .analyze import RegionTextModel
    from .formula_host import FormulaRecognizer
    from .table_unitable import Mi355UniTableStructure
    return FormulaRecognizer, RegionTextModel, Mi355UniTableStructure


def register_custom_models(base=None):
    """Registers the three seam models as virtual subclasses of `base` - default: `rapid_doc.model.custom.CustomBaseModel`, imported HERE and
    never at package import - and returns the base.  Idempotent.  ImportError when RapidDoc is not importable and no `base` is given."""
    if base is None:
        try:
            from rapid_doc.model.custom import CustomBaseModel as base
        except ImportError as e:
            raise ImportError("rapiddoc_amd.plugin.register_custom_models: rapid_doc.model.custom.CustomBaseModel is not importable "
                              f"({e}) - install RapidDoc next to this package, or pass the base class as `base=`") from e
    if not hasattr(base, "register"):
        raise TypeError(f"{base!r} has no register(): the base must be an abc.ABC like rapid_doc.model.custom.CustomBaseModel")
    names = [cls.__name__ for cls in seam_classes()]
    assert len(set(names)) == len(names), names              # the reference's registry keys custom models by class name
    for cls in seam_classes():
        base.register(cls)
    return base


def custom_configs(formula=None, ocr=None, table=None, base=None) -> dict:
    """{"formula_config": {"custom_model": formula}, "ocr_config": {...}, "table_config": {...}} with only the keys that were given, after
    `register_custom_models(base)`.  Builds nothing: the caller constructs the models, with the routes it wants (`host_images="stage"`)."""
    register_custom_models(base)
    given = (("formula_config", formula), ("ocr_config", ocr), ("table_config", table))
    return {key: {"custom_model": model} for key, model in given if model is not None}
