"""Host side of the table path behind the structure model (numpy only): what RapidTable runs after `table_structure(imgs)` and what
RapidTableModel.predict prepares in front of it.  Restated from the reference (paths relative to rapid_doc/model/table):

  format_ocr_results                         rapid_table_self/utils/utils.py
  TableMatch.filter_ocr_result / match_result / get_pred_html / decode_logic_points      rapid_table_self/table_matcher/main.py
  normalize_table_ocr_text / normalize_table_cell_text                                   utils.py
  the OCR-list preparation of RapidTableModel.predict (fill boxes, uuid rows, skipped inner text, formula / checkbox rows)   rapid_table.py:178-213

Kept as there: OCR boxes are matched in chunks of 256; an OCR box whose best IoU is below 0.1 ** 8 goes to no cell; among cells of equal
1 - IoU the one with the smallest corner distance wins and among those the lowest cell index."""
from __future__ import annotations

import html as _html
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MATCH_CHUNK = 256
MIN_IOU = 0.1 ** 8
INLINE_LEFT, INLINE_RIGHT = "$", "$"        # the reference's default inline formula delimiters (pipeline_middle_json_mkcontent.py)


# ------------------------------------------------------------------------------------------------------------------ OCR text
_WHOLE_TEXT = {"香": "否", "哦樂": "哦"}
_DIGIT_HAO = re.compile(r"^([0-9])號$")
_CJK = "\u3400-\u9fff"
_CJK_RE = re.compile(f"[{_CJK}]")
_CJK_PUNCT = "，。、“”‘’；：？！、：（）《》【】"
_LATIN = "A-Za-z0-9$"
_CELL_RULES = tuple(re.compile(p) for p in (
    rf"(?<=[{_CJK}])\s+(?=[{_CJK}])",
    rf"(?<=[{_CJK}{_LATIN}])\s+(?=[{_CJK_PUNCT}])",
    rf"(?<=[{_CJK_PUNCT}])\s+(?=[{_CJK}{_LATIN}])",
    rf"(?<=[{_LATIN}])\s+(?=[{_CJK}])",
    rf"(?<=[{_CJK}])\s+(?=[{_LATIN}])",
))


def normalize_table_ocr_text(text) -> str:
    """OCR text in front of the matcher: stripped, two whole-string recogniser slips mended, "<digit>號" -> "<digit>", HTML-escaped"""
    if text is None:
        return ""
    text = str(text).strip()
    text = _WHOLE_TEXT.get(text, text)
    m = _DIGIT_HAO.fullmatch(text)
    if m:
        text = m.group(1)
    return _html.escape(text)


def normalize_table_cell_text(text):
    """Cell text with CJK characters: the blanks OCR leaves between CJK characters, around CJK punctuation and between CJK and
    Latin / digit runs are removed, in the reference's five steps and their order.  Text without a CJK character is returned as it is."""
    if not text or not _CJK_RE.search(text):
        return text
    for rule in _CELL_RULES:
        text = rule.sub("", text)
    return text


# ------------------------------------------------------------------------------------------------------------------ OCR boxes
def format_ocr_results(ocr_result, img_h: int, img_w: int) -> Tuple[np.ndarray, List[Tuple[str, float]]]:
    """[quads [n,4,2], texts, scores] -> (boxes [n,4] = (x0, y0, x1, y1) clipped to the image, [(text, score)])"""
    rec = list(zip(ocr_result[1], ocr_result[2]))
    quads = np.array(ocr_result[0])
    lo = np.maximum(quads[..., :2].min(axis=1), 0)
    hi = np.minimum(quads[..., :2].max(axis=1), [img_w, img_h])
    return np.hstack([lo, hi]), rec


def points_to_bbox(points) -> list:
    """quad -> [x of corner 0, y of corner 0, x of corner 1, y of corner 2] (ocr_utils.points_to_bbox)"""
    return [points[0][0], points[0][1], points[1][0], points[2][1]]


def bbox_to_points(bbox) -> np.ndarray:
    x0, y0, x1, y1 = bbox
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]]).astype("float32")


def _inside(a, b) -> bool:
    return a[0] >= b[0] and a[1] >= b[1] and a[2] <= b[2] and a[3] <= b[3]


def fill_white(bgr: np.ndarray, bbox) -> None:
    """cv2.rectangle(img, (x0, y0), (x1, y1), white, thickness=-1) with int() corners: both corner pixels are inside, either corner order,
    clipped to the image"""
    xa, ya, xb, yb = (int(v) for v in bbox)
    x0, x1, y0, y1 = min(xa, xb), max(xa, xb), min(ya, yb), max(ya, yb)
    h, w = bgr.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    if x0 <= x1 and y0 <= y1:
        bgr[y0:y1 + 1, x0:x1 + 1] = 255


def prepare_ocr_list(bgr: np.ndarray, ocr_result: list, fill_image_res=None, mfd_res=None, skip_text_in_image: bool = True) -> list:
    """The list preparation of RapidTableModel.predict, IN PLACE on `bgr` and `ocr_result` = [boxes, texts, scores] (three lists):
    every fill image is whited out of the picture and appended as (its quad, its uuid, 1), the OCR rows that lie inside it are dropped
    when `skip_text_in_image`; then one row per formula (`latex` between the inline delimiters) or checkbox of `mfd_res`."""
    for fill in fill_image_res or []:
        box = points_to_bbox(fill["ocr_bbox"])
        fill_white(bgr, box)
        ocr_result[0].append(fill["ocr_bbox"])
        ocr_result[1].append(fill["uuid"])
        ocr_result[2].append(1)
        if skip_text_in_image:
            drop = [i for i, q in enumerate(ocr_result[0][:-1]) if _inside(points_to_bbox(q), box)]
            for i in reversed(drop):
                for col in ocr_result[:3]:
                    del col[i]
    for mfd in mfd_res or []:
        if mfd.get("latex"):
            text = normalize_table_ocr_text(f"{INLINE_LEFT}{mfd['latex']}{INLINE_RIGHT}")
        elif mfd.get("checkbox"):
            text = normalize_table_ocr_text(mfd["checkbox"])
        else:
            continue
        ocr_result[1].append(text)
        ocr_result[0].append(bbox_to_points(mfd["bbox"]))
        ocr_result[2].append(1)
    return ocr_result


# ------------------------------------------------------------------------------------------------------------------ the matcher
def filter_ocr_result(cell_bboxes: np.ndarray, dt_boxes, rec_res):
    """Drops the OCR boxes that end above the first cell.  With no cell the minimum of an empty array raises ValueError, as there."""
    top = cell_bboxes[:, 1::2].min()
    keep = [(b, r) for b, r in zip(dt_boxes, rec_res) if not np.max(b[1::2]) < top]
    return np.array([b for b, _ in keep]), [r for _, r in keep]


def _cells_xyxy(cell_bboxes) -> np.ndarray:
    """cell boxes with 4 or 8 numbers each -> [n,4] float64 (x0, y0, x1, y1)"""
    if cell_bboxes is None or np.asarray(cell_bboxes, dtype=object).size == 0:
        return np.empty((0, 4), dtype=np.float64)
    rows = []
    for c in cell_bboxes:
        c = np.asarray(c, dtype=np.float64).reshape(-1)
        if c.size == 8:
            rows.append([c[0::2].min(), c[1::2].min(), c[0::2].max(), c[1::2].max()])
        elif c.size == 4:
            rows.append(c.tolist())
        else:
            raise ValueError(f"Unsupported table cell bbox shape: {c.shape}")
    return np.asarray(rows, dtype=np.float64)


def _iou_and_distance(dt: np.ndarray, cells: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """[n,4] x [m,4] -> (IoU [n,m], corner distance [n,m]) in the reference's operation order"""
    d, c = dt[:, None, :], cells[None, :, :]
    area = (d[..., 2] - d[..., 0]) * (d[..., 3] - d[..., 1]) + (c[..., 2] - c[..., 0]) * (c[..., 3] - c[..., 1])
    y_lo, y_hi = np.maximum(d[..., 1], c[..., 1]), np.minimum(d[..., 3], c[..., 3])
    x_lo, x_hi = np.maximum(d[..., 0], c[..., 0]), np.minimum(d[..., 2], c[..., 2])
    inter = (y_hi - y_lo) * (x_hi - x_lo)
    union = area - inter
    iou = np.zeros_like(inter, dtype=np.float64)
    np.divide(inter, union, out=iou, where=(y_lo < y_hi) & (x_lo < x_hi) & (union != 0))
    d_tl = np.abs(c[..., 0] - d[..., 0]) + np.abs(c[..., 1] - d[..., 1])
    d_br = np.abs(c[..., 2] - d[..., 2]) + np.abs(c[..., 3] - d[..., 3])
    d_all = np.abs(c[..., 0] - d[..., 0]) + np.abs(c[..., 1] - d[..., 1]) + np.abs(c[..., 2] - d[..., 2]) + np.abs(c[..., 3] - d[..., 3])
    return iou, d_all + np.minimum(d_tl, d_br)


def match_result(cell_bboxes, dt_boxes, min_iou: float = MIN_IOU) -> Dict[int, List[int]]:
    """cell index -> the OCR rows assigned to it, in OCR order"""
    matched: Dict[int, List[int]] = {}
    dt = np.asarray(dt_boxes, dtype=np.float64)
    if dt.size == 0:
        return matched
    dt = dt.reshape(-1, 4)
    cells = _cells_xyxy(cell_bboxes)
    if cells.size == 0:
        return matched
    for start in range(0, len(dt), MATCH_CHUNK):
        iou, dist = _iou_and_distance(dt[start:start + MATCH_CHUNK], cells)
        inv = 1.0 - iou
        for row in range(inv.shape[0]):
            first = np.flatnonzero(inv[row] == inv[row].min())               # ascending cell index
            d = dist[row, first]
            best = int(first[np.flatnonzero(d == d.min())[0]])
            if 1.0 - iou[row, best] >= 1 - min_iou:
                continue
            matched.setdefault(best, []).append(start + row)
    return matched


_SECTION_TAGS = ("<thead>", "</thead>", "<tbody>", "</tbody>")


def get_pred_html(structure: Sequence[str], matched: Dict[int, List[int]], rec_res, cell_text=None) -> Tuple[str, List[str]]:
    """The structure tokens with the matched texts put into their cells.  Several texts in one cell: empties dropped, a leading blank and
    every <b> / </b> removed, stripped, joined by one blank; the cell is bold when the first text carried <b>.  `cell_text`: applied to
    every cell's joined text (Mi355RapidTable passes normalize_table_cell_text; the reference runs it over the finished HTML)."""
    out: List[str] = []
    td = 0
    for tag in structure:
        if "</td>" not in tag:
            out.append(tag)
            continue
        if tag == "<td></td>":
            out.append("<td>")
        if td in matched:
            rows = matched[td]
            many = len(rows) > 1
            bold = many and "<b>" in rec_res[rows[0]][0]
            if bold:
                out.append("<b>")
            parts = []
            for text in (rec_res[r][0] for r in rows):
                if many:
                    if len(text) == 0:
                        continue
                    if text[0] == " ":
                        text = text[1:]
                    text = text.replace("<b>", "").replace("</b>", "").strip()
                    if len(text) == 0:
                        continue
                parts.append(text)
            joined = " ".join(parts)
            out.append(cell_text(joined) if cell_text else joined)
            if bold:
                out.append("</b>")
        out.append("</td>" if tag == "<td></td>" else tag)
        td += 1
    out = [t for t in out if t not in _SECTION_TAGS]
    return "".join(out), out


def process_one(pred_struct, cell_bboxes: np.ndarray, dt_boxes, rec_res, cell_text=None) -> str:
    """TableMatch.process_one: pred_struct = (structure tokens, score)"""
    dt_boxes, rec_res = filter_ocr_result(cell_bboxes, dt_boxes, rec_res)
    return get_pred_html(pred_struct[0], match_result(cell_bboxes, dt_boxes), rec_res, cell_text)[0]


def match_tables(pred_structures, cell_bboxes, dt_boxes, rec_reses, cell_text=None) -> List[Optional[str]]:
    """TableMatch.__call__: one HTML string per table, None for a table without OCR input"""
    return [None if d is None or r is None else process_one(s, c, d, r, cell_text)
            for s, c, d, r in zip(pred_structures, cell_bboxes, dt_boxes, rec_reses)]


def decode_one_logic_points(structure: Sequence[str]) -> List[List[int]]:
    """Per cell [first row, last row, first column, last column] of the grid the spans lay out"""
    points: List[List[int]] = []
    taken = set()
    row = col = 0
    i = 0
    while i < len(structure):
        tok = structure[i]
        if tok == "<tr>":
            col = 0
        elif tok == "</tr>":
            row += 1
        elif tok.startswith("<td"):
            rowspan = colspan = 1
            if tok != "<td></td>":
                i += 1
                while i < len(structure) and not structure[i].startswith(">"):
                    if "colspan=" in structure[i]:
                        colspan = int(structure[i].split("=")[1].strip("\"'"))
                    elif "rowspan=" in structure[i]:
                        rowspan = int(structure[i].split("=")[1].strip("\"'"))
                    i += 1
            while (row, col) in taken:
                col += 1
            points.append([row, row + rowspan - 1, col, col + colspan - 1])
            taken.update((r, c) for r in range(row, row + rowspan) for c in range(col, col + colspan))
            col += colspan
        i += 1
    return points


def decode_logic_points(pred_structures) -> List[np.ndarray]:
    return [np.array(decode_one_logic_points(s[0])) for s in pred_structures]
