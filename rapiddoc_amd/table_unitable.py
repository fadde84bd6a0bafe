"""UniTable table-structure recogniser on the MI355X engine: the drop-in for the reference's `UniTableStructure`
(rapid_table_self/table_structure/unitable/main.py) - encoder (`unitable_encoder`), decoder and greedy loop (`unitable_decoder`,
rd_table_decode), and the host restatements of `decode_tokens`, `rescale_bboxes` and `wrap_with_html_struct`.

The token ids of the loop (prefix, eos, pad, `]</td>`, the bbox range) and the `id -> token` list come from the vocabulary file, which the
product does not ship: they are the caller's (`TableIds`, `id_to_token`); there is no `tokenizers` dependency.  `STAND_IN_IDS` /
`stand_in_tokens()` follow the order of the reference's VALID_HTML_BBOX_TOKENS (eos 1, the 49 HTML tokens 12 .. 60, bbox-0 .. bbox-448 =
61 .. 509, the module's 499 whitelisted ids) - a stand-in for tests, not a fact about the shipped file.

`Mi355RapidTable` is the whole table path around it, the drop-in for `RapidTableModel(model_type=UNITABLE)` (rapid_table.py): the
reference's pixels in front (`resize="pil"`, rd_preproc_resize_aa_norm), RapidTable's matcher behind (rapiddoc_amd/table_match.py)."""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

IMG_SIZE = 448
MAX_SEQ_LEN = 1024
MAX_BATCH = 8
MAX_SLOTS = 8                # RD_TABLE_STREAM_MAX_SLOTS
# pre_process.py: transforms.Normalize on the RGB image scaled to [0, 1]
NORM_MEAN = (0.86597056, 0.88463002, 0.87491087)
NORM_STD = (0.20686628, 0.18201602, 0.18485524)
TASK_TOKENS = ["[table]", "[html]", "[cell]", "[bbox]", "[cell+bbox]", "[html+bbox]"]
HTML_TOKENS = (["<td></td>", "<td>[", "]</td>", "<td", ">[", "></td>", "<tr>", "</tr>", "<tbody>", "</tbody>", "<thead>", "</thead>"]
               + [f' rowspan="{i}"' for i in range(2, 20)] + [f' colspan="{i}"' for i in range(2, 20)] + [' colspan="25"'])


@dataclass(frozen=True)
class TableIds:
    prefix: int
    eos: int
    pad: int
    bbox_close: int          # `]</td>`
    bbox_first: int          # bbox-0
    bbox_last: int           # bbox-448


STAND_IN_IDS = TableIds(prefix=11, eos=1, pad=2, bbox_close=14, bbox_first=61, bbox_last=509)


def stand_in_tokens() -> List[str]:
    """id -> token list of the stand-in vocabulary (960 entries)"""
    toks = [f"<unused-{i}>" for i in range(960)]
    toks[0], toks[1], toks[2] = "<bos>", "<eos>", "<pad>"
    for i, t in enumerate(TASK_TOKENS):
        toks[6 + i] = t
    for i, t in enumerate(HTML_TOKENS):
        toks[12 + i] = t
    for i in range(IMG_SIZE + 1):
        toks[61 + i] = f"bbox-{i}"
    return toks


class _Cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("prefix_id", "eos_id", "pad_id", "bbox_close_id", "bbox_first_id", "bbox_last_id")]


def cfg_struct(ids: TableIds) -> _Cfg:
    return _Cfg(ids.prefix, ids.eos, ids.pad, ids.bbox_close, ids.bbox_first, ids.bbox_last)


# ------------------------------------------------------------------------------------------------------------------ host restatements
def loop_reference(next_token, ids: TableIds, max_steps: int = MAX_SEQ_LEN) -> List[int]:
    """`UniTableStructure.loop_decode` for one table on the host: next_token(context) -> the decoder's whitelist argmax.  The counter
    rises with every bbox token, is cleared only when it exceeds 4 (the token is then replaced by `]</td>`), and no other token resets it."""
    ctx, count = [ids.prefix], 0
    for _ in range(max_steps):
        if ids.eos in ctx:
            break
        t = int(next_token(ctx))
        if ids.bbox_first <= t <= ids.bbox_last:
            count += 1
            if count > 4:
                t, count = ids.bbox_close, 0
        ctx.append(t)
    return ctx


_TR = re.compile(r"<tr>(.*?)</tr>", re.DOTALL)
_TD = re.compile(r"<td(.*?)>(.*?)</td>", re.DOTALL)
_BBOX = re.compile(r"\[ bbox-(\d+) bbox-(\d+) bbox-(\d+) bbox-(\d+) \]")


def decode_tokens(token_ids: Sequence[int], id_to_token: Sequence[str], joiner: str = " ") -> Tuple[np.ndarray, List[str]]:
    """main.py `decode_tokens`: the ids as one string (tokens joined by `joiner`, what the vocabulary's decode gives with the special tokens
    kept), then the three regexes.  As there, they run over the WHOLE string, not the part in front of <eos>.  Returns (bboxes float32
    [n, 8] = the four corners clockwise from the top left, zeros for a cell without a box; the html token list)."""
    pred_html = joiner.join(id_to_token[int(i)] for i in token_ids)
    decoded, boxes = [], []
    for tr in _TR.finditer(pred_html):
        decoded.append("<tr>")
        for td in _TD.finditer(tr.group(1)):
            attrs, content = td.group(1).strip(), td.group(2).strip()
            if attrs:
                decoded.append("<td")
                decoded.extend(" " + a for a in attrs.split())
                decoded.extend([">", "</td>"])
            else:
                decoded.append("<td></td>")
            m = _BBOX.search(content)
            if m:
                x0, y0, x1, y1 = map(int, m.groups())
                boxes.append(np.array([x0, y0, x1, y0, x1, y1, x0, y1]))
            else:
                boxes.append(np.array([0, 0, 0, 0, 0, 0, 0, 0]))
        decoded.append("</tr>")
    return np.array(boxes).astype(np.float32), decoded


def rescale_bboxes(ori_h: int, ori_w: int, bboxes: np.ndarray) -> np.ndarray:
    """post_process.py: 448-space corners to the original image, clipped; in place, as there"""
    bboxes[:, 0::2] *= ori_w / IMG_SIZE
    bboxes[:, 1::2] *= ori_h / IMG_SIZE
    bboxes[:, 0::2] = np.clip(bboxes[:, 0::2], 0, ori_w - 1)
    bboxes[:, 1::2] = np.clip(bboxes[:, 1::2], 0, ori_h - 1)
    return bboxes


def wrap_with_html_struct(structure: List[str]) -> List[str]:
    return ["<html>", "<body>", "<table>"] + structure + ["</table>", "</body>", "</html>"]


# ------------------------------------------------------------------------------------------------------------------ the class
class Mi355UniTableStructure:
    """`UniTableStructure` on the engine.  encoder / decoder: path to / bytes of a .safetensors file, or a state dict."""

    def __init__(self, encoder, decoder, ids: TableIds, id_to_token: Sequence[str], device: int = 0, max_new_tokens: int = MAX_SEQ_LEN,
                 resize: str = "linear", batching: str = "chunk", slots: int = MAX_SLOTS):
        """`resize`: "linear" = the engine's 2-tap linear resize (rd_preproc_resize_norm), "pil" = Pillow's antialiased bilinear, the
        reference's transforms.Resize on a PIL image, bit for bit (rd_preproc_resize_aa_norm).
        `batching`: "chunk" decodes every group of 8 tables as one batch, which runs until its longest table has ended; "stream" encodes
        the groups, then decodes all tables through `slots` (1 .. 8) decode rows that take the next waiting table as soon as theirs ends
        (`RdEngine.table_decode_stream`).  Both return the same contexts in the caller's order."""
        from .engine import RdEngine
        if resize not in ("linear", "pil"):
            raise ValueError("resize must be 'linear' or 'pil'")
        if batching not in ("chunk", "stream"):
            raise ValueError("batching must be 'chunk' or 'stream'")
        if isinstance(slots, bool) or not isinstance(slots, (int, np.integer)) or not 1 <= int(slots) <= MAX_SLOTS:
            raise ValueError(f"slots must be an integer in 1 .. {MAX_SLOTS}, got {slots!r}")
        self.batching, self.slots, self.last_stream_stats = batching, int(slots), []
        self.ids, self.id_to_token, self.max_new_tokens, self.resize = ids, list(id_to_token), int(max_new_tokens), resize
        self.encoder = RdEngine("unitable_encoder", device).load_weights(encoder)
        self.decoder = RdEngine("unitable_decoder", device).load_weights(decoder)
        self._dev = torch.device("cuda", device)

    def preprocess(self, imgs: list) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
        """BGR uint8 HWC images (numpy arrays or device tensors) -> normalised [B,3,448,448] on the device, every image written straight
        into its row of the batch with no host synchronisation in between.  resize="linear": the engine's linear resize (restated, not
        pinned); resize="pil": Pillow's antialiased bilinear, pinned to Pillow."""
        from .engine import preproc_resize_aa_norm, preproc_resize_norm
        imgs = [img for img in imgs if img is not None]
        x = torch.empty((len(imgs), 3, IMG_SIZE, IMG_SIZE), dtype=torch.float32, device=self._dev)
        if self.resize == "linear" and self.LINEAR_ROUTE == "sources" and len(imgs):
            return self._preprocess_linear_sources(imgs, x)
        shapes = []
        for i, img in enumerate(imgs):
            shapes.append(tuple(int(v) for v in img.shape[:2]))
            if isinstance(img, torch.Tensor):
                u8 = img.to(self._dev, non_blocking=True).contiguous()
            else:
                u8 = torch.from_numpy(np.ascontiguousarray(img)).to(self._dev, non_blocking=True)
            if self.resize == "pil":
                preproc_resize_aa_norm(u8, (IMG_SIZE, IMG_SIZE), mean=NORM_MEAN, std=NORM_STD, swap_rb=True, out=x[i])
            else:
                preproc_resize_norm(u8, (IMG_SIZE, IMG_SIZE), mean=NORM_MEAN, std=NORM_STD, swap_rb=True, out=x[i])
        return x, shapes

    LINEAR_ROUTE = "sources"           # "loop": one copy and one launch per table; profiles/mb_mixed_pages.txt (d) decides it

    def _preprocess_linear_sources(self, imgs: list, x: torch.Tensor) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
        """resize="linear" for all tables of a call at once: the host images staged by ONE pinned pack and ONE copy, then ONE
        rd_preproc_resize_norm_sources launch writes every table's row of `x` - the bits of the per-table loop."""
        from .engine import preproc_resize_norm_sources
        from .host_stage import HostImageStage
        shapes = [tuple(int(v) for v in img.shape[:2]) for img in imgs]
        host = [i for i, img in enumerate(imgs) if not isinstance(img, torch.Tensor)]
        srcs = [img if i in host else img.to(self._dev, non_blocking=True).contiguous() for i, img in enumerate(imgs)]
        if host:
            if getattr(self, "_stage", None) is None:
                self._stage = HostImageStage(self._dev)
            for i, v in zip(host, self._stage.upload([imgs[i] for i in host]).views):
                srcs[i] = v
        # (no `interp`: the same default as the loop's preproc_resize_norm call, so the two routes cannot drift apart)
        preproc_resize_norm_sources(srcs, [(IMG_SIZE, IMG_SIZE)] * len(srcs), mean=NORM_MEAN, std=NORM_STD, swap_rb=True, out=list(x))
        if host:
            self._stage.release()
        return x, shapes

    def decode_ids(self, x: torch.Tensor) -> List[List[int]]:
        """normalised [B,3,448,448] -> per table the context the reference's loop ends with (prefix ... eos)"""
        if self.batching == "stream":
            return self._decode_ids_stream(x)
        out: List[List[int]] = []
        for i in range(0, x.shape[0], MAX_BATCH):
            memory = self.encoder.table_encoder_forward(x[i:i + MAX_BATCH])
            ids, n = self.decoder.table_decode(memory, self.ids, self.max_new_tokens)
            ids = ids.cpu().numpy()
            out.extend(ids[b, :n[b]].tolist() for b in range(ids.shape[0]))
        return out

    def _decode_ids_stream(self, x: torch.Tensor) -> List[List[int]]:
        """batching="stream": encode in groups of 8 into one [N,S,768] buffer, decode every window of tables that fits the token limit
        with one `table_decode_stream`, cut the rows by `lens`."""
        from .engine import TABLE_STREAM_MAX_TOKENS
        self.last_stream_stats = []
        N = int(x.shape[0])
        if N == 0:
            return []
        memory = None
        for i in range(0, N, MAX_BATCH):
            m = self.encoder.table_encoder_forward(x[i:i + MAX_BATCH])
            if memory is None:
                memory = torch.empty((N,) + tuple(m.shape[1:]), dtype=torch.float32, device=m.device)
            memory[i:i + m.shape[0]] = m
        out: List[List[int]] = []
        for beg, end in stream_windows(N, int(memory.shape[1]), TABLE_STREAM_MAX_TOKENS):
            ids, lens, stats = self.decoder.table_decode_stream(memory[beg:end], self.ids, self.max_new_tokens, self.slots)
            self.last_stream_stats.append(stats)
            ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
            out.extend(ids[b, :int(lens[b])].tolist() for b in range(ids.shape[0]))
        return out

    def forward_tensor(self, x: torch.Tensor, ori_shapes: Optional[List[Tuple[int, int]]] = None):
        """The pinned path: (struct_list, total_bboxes) as the reference's __call__ returns them, from an already normalised tensor"""
        ori_shapes = ori_shapes or [(IMG_SIZE, IMG_SIZE)] * x.shape[0]
        return self.finish(self.decode_ids(x), ori_shapes)

    def finish(self, contexts: List[List[int]], ori_shapes: List[Tuple[int, int]]):
        """contexts of `decode_ids` -> (struct_list, total_bboxes): the host functions behind the loop"""
        struct_list, total_bboxes = [], []
        for ctx, (h, w) in zip(contexts, ori_shapes):
            bboxes, html = decode_tokens(ctx, self.id_to_token)
            total_bboxes.append(rescale_bboxes(h, w, bboxes) if len(bboxes) else bboxes)
            struct_list.append((wrap_with_html_struct(html), 1.0))
        return struct_list, total_bboxes

    def batch_predict(self, image_list: List[np.ndarray], **kwargs) -> List[str]:
        """The CustomBaseModel shape the page driver's table seam takes (`batch_predict(image_list, **kwargs) -> list[str]`): one HTML
        string per table crop - the structure alone, cells empty (matching OCR text into cells is RapidTable's matcher, not this model)."""
        structs, _ = self(list(image_list)) if len(image_list) else ([], [])
        return ["".join(s) for s, _score in structs]

    def __call__(self, imgs: List[np.ndarray]):
        x, shapes = self.preprocess(imgs)
        return self.forward_tensor(x, shapes)


def stream_windows(n: int, S: int, max_tokens: int) -> list:
    """(begin, end) windows over n tables of S memory rows each: as many tables per `table_decode_stream` call as its token limit takes
    (N * S <= max_tokens, i.e. max_tokens // S tables).  One table alone must fit."""
    if n <= 0:
        return []
    per = max_tokens // S
    if per < 1:
        raise ValueError(f"one table has {S} memory rows, the stream decode takes {max_tokens} per call")
    return [(b, min(n, b + per)) for b in range(0, n, per)]


# ------------------------------------------------------------------------------------------------------------------ the whole table path
@dataclass
class TableOutput:
    """What RapidTable.__call__ returns (RapidTableOutput), without the images and the timing"""
    pred_htmls: list
    cell_bboxes: list
    logic_points: list


class Mi355RapidTable:
    """`RapidTableModel(model_type=UNITABLE)` on the engine: the structure model with the reference's pixels (resize="pil"), RapidTable's
    matcher behind it (rapiddoc_amd/table_match.py) and the OCR-list preparation of RapidTableModel.predict in front.  It is a
    `predict`-shaped table model: analyze.PageAnalyzer runs it through `TableOcr` (seam S3).

    `structure`: a Mi355UniTableStructure built with resize="pil", or None with encoder / decoder / ids / id_to_token to build one."""

    def __init__(self, structure: Optional[Mi355UniTableStructure] = None, encoder=None, decoder=None, ids: Optional[TableIds] = None,
                 id_to_token: Optional[Sequence[str]] = None, device: int = 0, max_new_tokens: int = MAX_SEQ_LEN):
        if structure is None:
            structure = Mi355UniTableStructure(encoder, decoder, ids, id_to_token, device=device, max_new_tokens=max_new_tokens, resize="pil")
        if structure.resize != "pil":
            raise ValueError("Mi355RapidTable needs a structure model with resize='pil' (the reference's pixels)")
        self.structure = structure

    def __call__(self, bgr_images, ocr_results=None) -> TableOutput:
        """The non-UNET branch of RapidTable.__call__: bgr_images = list of BGR uint8 [h,w,3] (numpy or device tensors), ocr_results = per
        image [quads, texts, scores] or None (no OCR engine of our own: the cells of such a call stay unmatched, pred_htmls is empty)."""
        from . import table_match as TM
        if not isinstance(bgr_images, list):
            bgr_images = [bgr_images]
        pred_structures, cell_bboxes = self.structure(bgr_images)
        return self._match(bgr_images, ocr_results, pred_structures, cell_bboxes)

    def _match(self, bgr_images: list, ocr_results, pred_structures: list, cell_bboxes: list) -> TableOutput:
        """what `__call__` does behind the structure model"""
        from . import table_match as TM
        logic_points = TM.decode_logic_points(pred_structures)
        dt_boxes, rec_res = [], []
        if ocr_results is not None:
            if len(ocr_results) != len(bgr_images):
                raise ValueError(f"Batch size mismatch: {len(bgr_images)} images but {len(ocr_results)} OCR results")
            for img, res in zip(bgr_images, ocr_results):
                d, r = TM.format_ocr_results(res, int(img.shape[0]), int(img.shape[1]))
                dt_boxes.append(d)
                rec_res.append(r)
        htmls = TM.match_tables(pred_structures, cell_bboxes, dt_boxes, rec_res, cell_text=TM.normalize_table_cell_text)
        return TableOutput(htmls, list(cell_bboxes), logic_points)

    def predict(self, image, ocr_result=None, fill_image_res=None, mfd_res=None, skip_text_in_image=True, use_img2table=False,
                skip_table_orientation=None):
        """RapidTableModel.predict for ModelType.UNITABLE: RGB uint8 image + [quads, texts, scores] (three lists, extended in place as
        there) -> the table's HTML, or None (no OCR rows; anything the reference's try / except swallows, such as a structure without a
        cell).  The cell text goes through normalize_table_cell_text before the tokens are joined (the reference re-serialises the
        finished HTML through BeautifulSoup instead: restated, not pinned)."""
        bgr = self._front(image, ocr_result, fill_image_res, mfd_res, skip_text_in_image, use_img2table, skip_table_orientation)
        if bgr is None:
            return None                  # (the reference would run its own OCR engine first; the page driver always hands the rows over)
        try:
            return self([bgr], [ocr_result]).pred_htmls[0]
        except Exception:                # as the reference: logged there, None here
            return None

    def _front(self, image, ocr_result=None, fill_image_res=None, mfd_res=None, skip_text_in_image=True, use_img2table=False,
               skip_table_orientation=None):
        """`predict` in front of the structure model: the switches that are not built raise, the OCR list is prepared in place; returns
        the BGR image, or None when there are no OCR rows"""
        from . import table_match as TM
        if use_img2table:
            raise NotImplementedError("use_img2table=True needs the img2table route and an OCR engine of RapidOcrTable's shape, which are not part of this package")
        bgr = np.ascontiguousarray(np.asarray(image)[:, :, ::-1])                # cv2.cvtColor(RGB2BGR): a copy, the caller's image stays
        if skip_table_orientation is None:
            skip_table_orientation = ocr_result is not None
        h, w = bgr.shape[:2]
        if (h / w if w > 0 else 1.0) > 1.2 and not skip_table_orientation:
            raise NotImplementedError("the portrait-rotation check needs a text detector on the table image (ocr_engine.ocr(rec=False)); "
                                      "pass an ocr_result or skip_table_orientation=True")
        if not ocr_result:
            return None
        TM.prepare_ocr_list(bgr, ocr_result, fill_image_res, mfd_res, skip_text_in_image)
        return bgr

    def predict_many(self, items: Sequence[tuple]) -> list:
        """`[self.predict(*it) for it in items]` with ONE structure call over every table that has OCR rows (so that a structure model
        built with batching="stream" sees the page batch's tables together); the matcher runs per table, each table under the same
        try / except -> None as in `predict`.  If the pooled structure call itself raises, every table goes the way `predict` takes it."""
        results: list = [None] * len(items)
        live = []                        # (index, bgr, ocr_result) of the tables that reach the structure model
        for i, it in enumerate(items):
            bgr = self._front(*it)
            if bgr is not None:
                live.append((i, bgr, it[1]))
        if not live:
            return results
        try:
            x, shapes = self.structure.preprocess([bgr for _i, bgr, _o in live])
            contexts = self.structure.decode_ids(x)
            if len(contexts) != len(live):
                raise RuntimeError("the structure model returned another number of tables")
        except Exception:
            contexts = None
        for k, (i, bgr, ocr_result) in enumerate(live):
            try:
                if contexts is None:
                    results[i] = self([bgr], [ocr_result]).pred_htmls[0]
                else:
                    structs, boxes = self.structure.finish([contexts[k]], [shapes[k]])
                    results[i] = self._match([bgr], [ocr_result], structs, boxes).pred_htmls[0]
            except Exception:            # as `predict`
                results[i] = None
        return results

    def batch_predict(self, images: list, ocr_result=None, fill_image_res=None, mfd_res=None, skip_text_in_image=True, use_img2table=False,
                      skip_table_orientation=None) -> list:
        return [self.predict(im, ocr_result, fill_image_res, mfd_res, skip_text_in_image, use_img2table, skip_table_orientation) for im in images]
