#!/usr/bin/env python3
"""Mint the fixtures of the table path behind and in front of the UniTable networks: Pillow's antialiased resample, RapidTable's matcher,
the OCR-list preparation of RapidTableModel.predict, and one end-to-end expectation on a PIL-preprocessed crop.

Runs only in the build container (it imports the reference tree and Pillow); what it writes next to itself is data only:

    table_path_resample.npz            per case `<name>_in` (uint8 [H, W, 3], noise of tests/table_path_reference.lcg_bytes) or `<name>_recipe`
                                       (seed, H, W of weights.synth_table_crop), `<name>_out` = (OH, OW) and `<name>_exp` = what
                                       PIL.Image.fromarray(in).resize((OW, OH), Image.BILINEAR) returns; `names` lists the small cases
    table_path_resample_448_{600x1000,120x300}.npz     the same for the two cases at the real target 448 x 448 (one file each: size limit)
    table_path_match.json              matcher cases (structure tokens, cell boxes, OCR list, image size -> HTML and logic points, from the
                                       reference's TableMatch / format_ocr_results), `predict_prep` (the image and the OCR list that
                                       RapidTableModel.predict hands to its table model) and `engine_inject` (recorded ids that hold cells
                                       -> the reference's decode_tokens / rescale_bboxes / wrap_with_html_struct -> TableMatch)
    summary_table_path.json            Pillow's version, the stand-ins used, the sizes, and `class_pil`: the reference encoder on the
                                       PIL-preprocessed 600 x 1000 crop, the loop around the reference decoder (EOS variant, LOOP_RULES of
                                       make_golden_unitable.py), decode_tokens, rescale_bboxes, wrap_with_html_struct

Stand-ins (packages that are absent here), as in the other mints: cv2.cvtColor(BGR2RGB / RGB2BGR) = channel flip; cv2.rectangle(thickness
-1) = table_match.fill_white (both corner pixels inside); transforms.Resize = PIL.Image.resize(BILINEAR) - which is what torchvision calls
for a PIL image; ToTensor / Normalize = ((u8.float() / 255) - mean) / std in torch fp32; normalize_table_html_cell_text (BeautifulSoup) =
identity, so every fixture text is one the reference returns unchanged (no CJK text with inner blanks); loguru's logger = a stub.
Pillow itself is real.

    python tests/golden/make_golden_table_path.py
"""
import ast
import html
import importlib.util
import json
import re
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(HERE))

import make_golden_unitable as MU  # noqa: E402
import table_path_reference as TP  # noqa: E402
from rapiddoc_amd import table_match as TM  # noqa: E402
from rapiddoc_amd import table_unitable as TU  # noqa: E402
from rapiddoc_amd import weights as W  # noqa: E402

REF_TABLE = MU.REF / "rapid_doc/model/table"
LIMIT = 1 << 20
SMALL = (("down_down", 53, 131), ("up_up", 9, 11), ("v_skipped", 24, 97), ("h_skipped", 61, 40), ("identity", 24, 40), ("up_down10", 5, 400),
         ("one_pixel", 1, 1))
SMALL_OUT = (24, 40)
BIG = ((600, 1000), (120, 300))
CROP_SEED = 1


def pil_resize(a, oh, ow):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))


def mint_resample(summary):
    import PIL
    out = {"names": np.array([n for n, _, _ in SMALL])}
    for i, (name, h, w) in enumerate(SMALL):
        a = TP.lcg_bytes(100 + i, (h, w, 3))
        out[name + "_in"], out[name + "_out"], out[name + "_exp"] = a, np.array(SMALL_OUT, dtype=np.int64), pil_resize(a, *SMALL_OUT)
    fn = HERE / "table_path_resample.npz"
    np.savez_compressed(fn, **out)
    sizes = {fn.name: fn.stat().st_size}
    for h, w in BIG:
        name = f"{h}x{w}"
        a = W.synth_table_crop(CROP_SEED, h, w)
        fn = HERE / f"table_path_resample_448_{name}.npz"
        np.savez_compressed(fn, names=np.array([name]), **{name + "_recipe": np.array([CROP_SEED, h, w], dtype=np.int64),
                                                          name + "_out": np.array([448, 448], dtype=np.int64), name + "_exp": pil_resize(a, 448, 448)})
        sizes[fn.name] = fn.stat().st_size
    assert all(v <= LIMIT for v in sizes.values()), sizes
    summary["pillow"] = PIL.__version__
    summary["resample_bytes"] = sizes
    print("resample", sizes)


# ---------------------------------------------------------------------------------------------------------------- reference pieces
def load_table_match():
    """the reference's table_matcher package by path (it imports numpy and its own utils only)"""
    d = REF_TABLE / "rapid_table_self/table_matcher"
    spec = importlib.util.spec_from_file_location("ref_table_matcher", d / "__init__.py", submodule_search_locations=[str(d)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_table_matcher"] = mod
    spec.loader.exec_module(mod)
    return mod.TableMatch()


def extract(path, names, ns, assigns=()):
    """exec the named functions (annotations dropped) and module-level assignments of a reference file in `ns`"""
    tree = ast.parse(Path(path).read_text())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id in assigns for t in node.targets):
            exec(compile(ast.Module([node], []), str(path), "exec"), ns)
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in names:
            node.returns = None
            for a in node.args.args:
                a.annotation = None
            exec(compile(ast.Module([node], []), str(path), "exec"), ns)
    return ns


def reference_namespace():
    ns = {"np": np, "re": re, "html": html, "Tuple": tuple, "List": list}
    extract(REF_TABLE / "rapid_table_self/utils/utils.py", ("format_ocr_results",), ns)
    extract(REF_TABLE / "utils.py", ("normalize_table_ocr_text", "normalize_table_cell_text"), ns,
            ("TABLE_OCR_REC_SINGLE_CHAR_REPLACEMENTS", "TABLE_OCR_REC_REGEX_REPLACEMENTS", "CJK_RE", "CJK_PUNCT_RE"))
    extract(MU.REF / "rapid_doc/utils/ocr_utils.py", ("points_to_bbox", "bbox_to_points"), ns)
    extract(MU.REF / "rapid_doc/utils/boxbase.py", ("is_in",), ns)
    return ns


def quad(x0, y0, x1, y1):
    return [[float(x0), float(y0)], [float(x1), float(y0)], [float(x1), float(y1)], [float(x0), float(y1)]]


def corners8(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def match_cases():
    """name -> (structure tokens without the html wrapper, cell boxes, [quads, texts, scores], (img_h, img_w))"""
    grid = ["<tr>", "<td></td>", "<td></td>", "</tr>", "<tr>", "<td></td>", "<td></td>", "</tr>"]
    cells4 = [[0, 0, 100, 50], [100, 0, 200, 50], [0, 50, 100, 100], [100, 50, 200, 100]]
    cases = {}
    cases["spans_8pt"] = (
        ["<thead>", "<tr>", "<td", ' rowspan="2"', ">", "</td>", "<td", ' colspan="2"', ">", "</td>", "</tr>", "</thead>", "<tbody>", "<tr>", "<td></td>",
         "<td></td>", "</tr>", "<tr>", "<td", ' rowspan="2"', ' colspan="2"', ">", "</td>", "<td></td>", "</tr>", "<tr>", "<td></td>", "</tr>", "</tbody>"],
        [corners8(0, 0, 60, 80), corners8(60, 0, 200, 40), corners8(60, 40, 130, 80), corners8(130, 40, 200, 80), corners8(0, 80, 130, 160),
         corners8(130, 80, 200, 120), corners8(130, 120, 200, 160)],
        [[quad(5, 10, 50, 70), quad(70, 5, 190, 35), quad(65, 45, 120, 75), quad(140, 45, 195, 75), quad(10, 90, 120, 150), quad(135, 125, 195, 155)],
         ["name", "2023 &amp; 2024", "a", "b", "total", "9.5"], [0.99, 0.98, 0.97, 0.96, 0.95, 0.94]], (160, 200))
    cases["several_in_one_cell_bold"] = (
        grid, cells4,
        [[quad(5, 5, 45, 20), quad(50, 5, 95, 20), quad(5, 25, 60, 45), quad(110, 10, 190, 40), quad(10, 60, 90, 90), quad(110, 55, 150, 70), quad(110, 75, 190, 95)],
         ["<b>Head</b>", " of ", "", "plain", "<b>single</b>", " first ", "<b>second</b>"], [0.9] * 7], (100, 200))
    cases["above_first_cell_and_under_iou"] = (
        grid, [[0, 40, 100, 90], [100, 40, 200, 90], [0, 90, 100, 140], [100, 90, 1000, 1000]],
        [[quad(10, 5, 90, 30), quad(10, 45, 90, 85), quad(999.9999, 999.9999, 2000, 2000), quad(300, 10, 400, 41), quad(120, 100, 180, 130)],
         ["caption above", "kept", "sliver", "beside", "inside"], [0.9, 0.8, 0.7, 0.6, 0.5]], (2000, 2000))
    cases["equal_iou_decided_by_distance"] = (
        grid, [[0, 0, 100, 50], [100, 5, 200, 55], [0, 60, 100, 110], [100, 60, 200, 110]],
        [[quad(80, 10, 120, 40), quad(80, 70, 120, 100)], ["nearer the second", "lowest index"], [0.9, 0.9]], (110, 200))
    n = 300
    many_q = [quad(2 + 10 * (i % 20), 2 + 6 * (i // 20), 9 + 10 * (i % 20), 6 + 6 * (i // 20)) for i in range(n)]
    many_struct = sum((["<tr>"] + ["<td></td>"] * 4 + ["</tr>"] for _ in range(3)), [])
    many_cells = [[50 * c, 30 * r, 50 * c + 50, 30 * r + 30] for r in range(3) for c in range(4)]
    cases["more_than_256_boxes"] = (many_struct, many_cells, [many_q, [f"w{i}" for i in range(n)], [0.5] * n], (90, 200))
    cases["four_point_cells_int_boxes"] = (
        grid, cells4, [[[[3, 4], [90, 6], [88, 44], [2, 42]], [[-5, 60], [230, 58], [231, 130], [-4, 131]]], ["tilted", "wide clipped"], [0.9, 0.8]], (100, 200))
    return cases


def mint_match(ns):
    tm = load_table_match()
    rec = {}
    for name, (structure, cells, ocr, hw) in match_cases().items():
        wrapped = TU.wrap_with_html_struct(list(structure))
        cell_arr = np.array(cells, dtype=np.float32)
        dt, rr = ns["format_ocr_results"](ocr, hw[0], hw[1])
        html_ = tm([(wrapped, 1.0)], [cell_arr], [dt], [rr])[0]
        logic = tm.decode_logic_points([(wrapped, 1.0)])[0]
        assert html_ == TM.match_tables([(wrapped, 1.0)], [cell_arr], *[[v] for v in TM.format_ocr_results(ocr, hw[0], hw[1])])[0], name
        assert html_.count("</td>") == len(cells), name
        rec[name] = {"structure": wrapped, "cell_bboxes": cells, "ocr_result": ocr, "img_hw": list(hw), "dt_boxes": np.asarray(dt).tolist(), "html": html_,
                     "logic_points": logic.tolist()}
        print("match", name, html_[:160])
    assert "<td><b>Head of</b></td>" in rec["several_in_one_cell_bold"]["html"]
    assert "caption above" not in rec["above_first_cell_and_under_iou"]["html"] and "sliver" not in rec["above_first_cell_and_under_iou"]["html"]
    return rec, tm


def mint_predict_prep(ns):
    """RapidTableModel.predict itself (the method's own code, executed with stand-ins for cv2 / loguru / BeautifulSoup) with a table model
    that records what it is handed"""
    seen = {}

    class Cv2:
        COLOR_RGB2BGR, ROTATE_90_CLOCKWISE = 4, 0

        @staticmethod
        def cvtColor(a, code):
            return np.ascontiguousarray(np.asarray(a)[:, :, ::-1])

        @staticmethod
        def rectangle(img, p0, p1, color, thickness=-1):
            assert thickness == -1 and tuple(color) == (255, 255, 255)
            TM.fill_white(img, [p0[0], p0[1], p1[0], p1[1]])

    class Logger:
        def exception(self, e):
            seen["exception"] = repr(e)

    class ModelType:
        UNET_SLANET_PLUS, UNET_SLANET1M, UNET_UNITABLE, UNITABLE = "a", "b", "c", "unitable"

    class Out:
        pred_htmls = ["<html><body><table><tr><td>recorded</td></tr></table></body></html>"]

    class Self:
        model_type = ModelType.UNITABLE
        ocr_engine = None

        @staticmethod
        def table_model(bgr_images, ocr_results):
            seen["bgr"], seen["ocr"] = bgr_images[0].copy(), json.loads(json.dumps(ocr_results[0], default=lambda a: np.asarray(a).tolist()))
            return Out()

    pns = dict(ns, cv2=Cv2, logger=Logger(), ModelType=ModelType, inline_left_delimiter="$", inline_right_delimiter="$",
               normalize_table_html_cell_text=lambda s: s)
    tree = ast.parse((REF_TABLE / "rapid_table.py").read_text())
    fn = [n for c in tree.body if isinstance(c, ast.ClassDef) and c.name == "RapidTableModel" for n in c.body if isinstance(n, ast.FunctionDef) and n.name == "predict"][0]
    exec(compile(ast.Module([fn], []), "rapid_table.py", "exec"), pns)
    predict = pns["predict"]

    def img():
        a = np.full((40, 60, 3), 7, dtype=np.uint8)
        a[:, :, 1], a[:, :, 2] = 90, 180            # RGB in = (7, 90, 180)
        return a

    def ocr():
        return [[quad(2, 2, 20, 10), quad(22, 12, 30, 18), quad(40, 5, 58, 15), quad(5, 25, 25, 35)], ["a", "in the image", "c", "partly in"], [0.9, 0.8, 0.7, 0.6]]
    fills = [{"ocr_bbox": quad(20, 10, 35, 30), "uuid": "uuid-0001"}, {"ocr_bbox": [[50.7, 30.2], [57.9, 30.2], [57.9, 38.6], [50.7, 38.6]], "uuid": "uuid-0002"}]
    mfds = [{"bbox": [1, 30, 12, 38], "latex": "a<b"}, {"bbox": [30, 32, 40, 39], "checkbox": "☑"}, {"bbox": [0, 0, 1, 1]}, {"bbox": [44, 20, 50, 26], "latex": "", "checkbox": " x "}]
    cases = {"plain": {}, "fill_skip": {"fill_image_res": fills}, "fill_keep": {"fill_image_res": fills, "skip_text_in_image": False},
             "formulas": {"mfd_res": mfds}, "fill_and_formulas": {"fill_image_res": fills[:1], "mfd_res": mfds[:2]}}
    rec = {}
    for name, kw in cases.items():
        seen.clear()
        o = ocr()
        got = predict(Self(), img(), o, kw.get("fill_image_res"), kw.get("mfd_res"), kw.get("skip_text_in_image", True), False, None)
        assert got == Out.pred_htmls[0] and "exception" not in seen, (name, seen.get("exception"))
        white = np.argwhere((seen["bgr"] == 255).all(axis=2))
        rec[name] = {"kwargs": kw, "image_rgb": [7, 90, 180], "image_hw": [40, 60], "ocr_in": ocr(), "ocr_out": seen["ocr"], "white_pixels": int(len(white)),
                     "white_box_yx": [white.min(axis=0).tolist(), white.max(axis=0).tolist()] if len(white) else None,
                     "bgr_corner": seen["bgr"][0, 0].tolist()}
        print("predict_prep", name, rec[name]["ocr_out"][1], rec[name]["white_pixels"])
    for empty in (None, []):
        seen.clear()
        Self.ocr_engine = type("E", (), {"ocr": staticmethod(lambda *a, **k: [None])})()
        assert predict(Self(), img(), empty, None, None, True, False, True) is None and "ocr" not in seen
    return rec


# ---------------------------------------------------------------------------------------------------------------- the networks
def pil_preprocess(bgr):
    """TablePreprocess.preprocess_img with the stand-ins of the module docstring -> [1, 3, 448, 448] float32"""
    u8 = torch.from_numpy(pil_resize(np.ascontiguousarray(bgr[:, :, ::-1]), 448, 448).copy())
    mean, std = torch.tensor(TU.NORM_MEAN, dtype=torch.float32), torch.tensor(TU.NORM_STD, dtype=torch.float32)
    return ((u8.float() / 255 - mean) / std).permute(2, 0, 1)[None].contiguous()


def mint_class_pil(tm, host):
    torch.manual_seed(0)
    torch.set_num_threads(8)
    spec = importlib.util.spec_from_file_location("unitable_modules_ref", MU.MODULES)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ids = TU.STAND_IN_IDS
    enc, dec = mod.Encoder(), mod.GPTFastDecoder()
    man = lambda net: [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in net.state_dict().items()]
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in W.synth_state_dict(man(enc), MU.SEED).items()}, strict=True)
    base = W.synth_state_dict(man(dec), MU.SEED)
    enc.eval(), dec.eval()
    white = np.array(sorted(dec.token_white_list))
    got = {}
    dec.generator.register_forward_hook(lambda m, a, o: got.__setitem__("logits", o.detach()[:, -1].clone()))

    def load(state):
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)

    def loop(memory, the_ids, steps):
        dec.setup_caches(max_batch_size=1, max_seq_length=1024, dtype=torch.float32, device="cpu")
        lg = []

        def nt(ctx):
            with torch.no_grad():
                t = int(dec(torch.from_numpy(memory)[None], torch.tensor([ctx], dtype=torch.int32))[0, 0])
            lg.append(got["logits"][0].numpy())
            return t
        return TU.loop_reference(nt, the_ids, steps), np.stack(lg)

    ids_no = TU.TableIds(ids.prefix, -1, ids.pad, ids.bbox_close, ids.bbox_first, ids.bbox_last)
    found = None
    for seed in range(CROP_SEED, CROP_SEED + 40):
        crop = W.synth_table_crop(seed, 600, 1000)
        x = pil_preprocess(crop)
        with torch.no_grad():
            mem = enc(x).numpy()[0]
        load(base)
        _, L = loop(mem, ids_no, 61)
        m, g_ = L[:, white[1:]].max(axis=1) - L[:, ids.eos], MU.whitelist_gap(L, white[1:])
        cand = np.unique(m)
        for m_thr, g_thr in MU.LOOP_RULES:
            for beta in (cand[:-1] + cand[1:]) / 2:
                stop = int(np.argmax(m < beta)) if (m < beta).any() else -1
                if 20 <= stop <= 60 and np.abs(m[:stop + 1] - beta).min() > m_thr and g_[:stop].min() > g_thr:
                    found = (float(beta), stop, (m_thr, g_thr))
                    break
            if found:
                break
        print("class_pil search: crop seed", seed, "found", found, flush=True)
        if found:
            break
    assert found, "no EOS offset stops the table inside [20, 60] under LOOP_RULES"
    st = dict(base)
    st["generator.bias"] = base["generator.bias"].copy()
    st["generator.bias"][ids.eos] += np.float32(found[0])
    load(st)
    ctx, _ = loop(mem, ids, 64)
    assert len(ctx) - 2 == found[1] and ctx[-1] == ids.eos
    boxes, html_ = host["decode_tokens"](host["Self"](), torch.tensor([ctx]))
    wrapped = host["wrap_with_html_struct"](list(html_))
    ocr = [[quad(100, 100, 300, 140), quad(400, 300, 700, 340)], ["alpha", "beta"], [0.9, 0.8]]
    try:                                                    # what RapidTable.__call__ does next, inside RapidTableModel.predict's try / except
        rescaled = host["rescale_bboxes"](600, 1000, boxes.copy())
        dt, rr = TM.format_ocr_results(ocr, 600, 1000)
        predicted = tm([(wrapped, 1.0)], [rescaled], [dt], [rr])[0]
    except Exception as e:
        print("class_pil: the reference path raises", repr(e), "-> predict returns None")
        rescaled, predicted = boxes, None
    return {"crop_seed": seed, "crop_hw": [600, 1000], "bias_add": found[0], "rule": list(found[2]), "ids": ctx, "html": html_, "wrapped": wrapped,
            "boxes": np.asarray(rescaled).tolist(), "x_absmax": float(x.abs().max()), "x_mean": float(x.mean()), "ocr_result": ocr, "predict": predicted}


def mint_engine_inject(tm, host):
    """ids (stand-in vocabulary) that hold cells -> the reference's host functions -> TableMatch on a 600 x 1000 crop"""
    toks = TU.stand_in_tokens()
    t = {s_: i for i, s_ in enumerate(toks)}
    bb = lambda *v: [t[f"bbox-{x}"] for x in v]
    ids_ = [11, t["<tr>"], t["<td>["], *bb(10, 20, 200, 100), t["]</td>"], t["<td>["], *bb(210, 20, 440, 100), t["]</td>"], t["</tr>"], t["<tr>"], t["<td"],
            t[' colspan="2"'], t[">["], *bb(10, 110, 440, 300), t["]</td>"], t["</tr>"], 1]
    boxes, html_ = host["decode_tokens"](host["Self"](), torch.tensor([ids_]))
    wrapped = host["wrap_with_html_struct"](list(html_))
    cells = host["rescale_bboxes"](600, 1000, boxes.copy())
    ocr = [[quad(40, 40, 400, 120), quad(500, 35, 950, 125), quad(100, 200, 600, 260), quad(620, 300, 900, 380), quad(10, 2, 300, 20)],
           ["Item", "Price &lt; 5", "wide cell", "second line", "title above"], [0.9, 0.9, 0.8, 0.8, 0.7]]
    dt, rr = TM.format_ocr_results(ocr, 600, 1000)
    html_out = tm([(wrapped, 1.0)], [cells], [dt], [rr])[0]
    print("engine_inject", html_out)
    return {"ids": ids_, "ori_hw": [600, 1000], "wrapped": wrapped, "cell_bboxes": cells.tolist(), "ocr_result": ocr, "html": html_out,
            "logic_points": tm.decode_logic_points([(wrapped, 1.0)])[0].tolist()}


def main():
    summary = {"stand_ins": {"cv2.cvtColor": "channel flip", "cv2.rectangle": "table_match.fill_white", "transforms.Resize": "PIL.Image.resize(BILINEAR)",
                             "ToTensor/Normalize": "((u8.float() / 255) - mean) / std, torch fp32", "normalize_table_html_cell_text": "identity (bs4 absent)",
                             "loguru.logger": "stub"}}
    mint_resample(summary)
    ns = reference_namespace()
    for text in ("a &amp; b", " 5號 ", "香", "10號", "<b>x</b>", None, 7):
        assert ns["normalize_table_ocr_text"](text) == TM.normalize_table_ocr_text(text), text
    match, tm = mint_match(ns)
    host = MU.mint_host(TU)[1]
    out = {"cases": match, "predict_prep": mint_predict_prep(ns), "engine_inject": mint_engine_inject(tm, host)}
    (HERE / "table_path_match.json").write_text(json.dumps(out, indent=1, ensure_ascii=False))
    summary["class_pil"] = mint_class_pil(tm, host)
    (HERE / "summary_table_path.json").write_text(json.dumps(summary, indent=1))
    print("class_pil", {k: summary["class_pil"][k] for k in ("crop_seed", "bias_add", "rule", "html", "predict")}, "tokens", len(summary["class_pil"]["ids"]))


if __name__ == "__main__":
    main()
