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

The OCR-MODEL seam sits one level below `ocr_config['custom_model']`: the object `ocr_model_init()` returns, which RapidDoc's own driver
wraps with its text-layer mode, box merging, table OCR and score demotion (rapiddoc_amd/ocr_model.py).  `install_ocr_model` puts the
engine there:

    uninstall = plugin.install_ocr_model(pipeline)           # or {lang: pipeline}; device_crops=True: text lines are cut on the device
    doc_analyze(...)                                         # every ocr_model_init() call now builds a Mi355RapidOcrModel
    uninstall()
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


_INSTALLED: dict = {}       # id(model_init module) -> (module, uninstall)


def install_ocr_model(pipelines, device_crops: bool = False, module=None):
    """Replaces `rapid_doc.backend.pipeline.model_init.ocr_model_init` by a factory that builds `ocr_model.Mi355RapidOcrModel(pipelines,
    ...)` from the six arguments `atom_model_init` passes (det_db_box_thresh, lang, ocr_config, det_db_unclip_ratio,
    enable_merge_det_boxes, is_seal); a request with `is_seal=True` goes to the ORIGINAL function, so seals keep working through the
    reference's own model.  `pipelines`: a `PagePipeline` or {language: PagePipeline}.

    `device_crops=True` also replaces `get_rotate_crop_image` - the module global of `rapid_doc.utils.ocr_utils` that
    `get_ocr_result_list` looks up, and the name imported into `rapid_doc.backend.pipeline.analyze_utils` - by
    `ocr_model.lazy_crop_function(original)`: text lines become `LazyLineCrop`s and are cut on the device inside `ocr(list, det=False)`.

    `module`: the `model_init` module (tests pass a stand-in); default: imported HERE, never at package import - as are `ocr_utils` and
    `analyze_utils`, found next to it in `sys.modules` / by import.  Idempotent: a second call on an installed module changes nothing
    and returns the first call's `uninstall`, which puts back every attribute it replaced, by identity."""
    import importlib
    from . import ocr_model
    if module is None:
        try:
            module = importlib.import_module("rapid_doc.backend.pipeline.model_init")
        except ImportError as e:
            raise ImportError(f"rapiddoc_amd.plugin.install_ocr_model: rapid_doc.backend.pipeline.model_init is not importable ({e}) - "
                              "install RapidDoc next to this package, or pass the module as `module=`") from e
    if id(module) in _INSTALLED and _INSTALLED[id(module)][0] is module:
        return _INSTALLED[id(module)][1]
    original = module.ocr_model_init

    def ocr_model_init(det_db_box_thresh=0.5, lang=None, ocr_config=None, det_db_unclip_ratio=1.8, enable_merge_det_boxes=True, is_seal=False):
        if is_seal:
            return original(det_db_box_thresh, lang, ocr_config, det_db_unclip_ratio, enable_merge_det_boxes, is_seal)
        return ocr_model.Mi355RapidOcrModel(pipelines, det_db_box_thresh=det_db_box_thresh, lang=lang, ocr_config=ocr_config, use_dilation=True,
                                            det_db_unclip_ratio=det_db_unclip_ratio, enable_merge_det_boxes=enable_merge_det_boxes, is_seal=False)
    ocr_model_init.rapiddoc_amd_original = original

    touched = [(module, "ocr_model_init", original)]
    module.ocr_model_init = ocr_model_init
    if device_crops:
        root = module.__name__.rsplit(".backend.pipeline.", 1)[0] if ".backend.pipeline." in module.__name__ else "rapid_doc"
        try:
            utils = importlib.import_module(root + ".utils.ocr_utils")
            users = [importlib.import_module(root + ".backend.pipeline.analyze_utils")]
        except ImportError as e:
            module.ocr_model_init = original
            raise ImportError(f"rapiddoc_amd.plugin.install_ocr_model(device_crops=True): {e}") from e
        crop_original = utils.get_rotate_crop_image
        lazy = ocr_model.lazy_crop_function(crop_original)
        for mod in [utils] + users:
            if getattr(mod, "get_rotate_crop_image", None) is crop_original:
                touched.append((mod, "get_rotate_crop_image", crop_original))
                setattr(mod, "get_rotate_crop_image", lazy)

    def uninstall() -> None:
        for mod, name, value in reversed(touched):
            setattr(mod, name, value)
        touched.clear()
        _INSTALLED.pop(id(module), None)

    _INSTALLED[id(module)] = (module, uninstall)
    return uninstall
