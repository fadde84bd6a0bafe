"""GPU: a page batch gives the same quads, strings and scores whether the host stages between its GPU stages run in the library
(the default) or as the Python restatements (`PagePipeline.host_native = False`, what RD_HOST_NATIVE=0 selects)."""
import numpy as np
import pytest
import torch

from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu


def test_page_batch_is_the_same_with_the_host_stages_in_the_library_and_in_python(golden_dir):
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline, render_text_maps
    states = {k: W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}
    pipe = PagePipeline(states, n_rec_streams=2)
    assert pipe.host_native
    pages_np, boxes = synth_batch(11, 2)
    pages = torch.from_numpy(pages_np).cuda()
    maps = render_text_maps(boxes, pages_np.shape[1:3], pipe.det_preprocess(pages[:1])[1], pages.device)

    def run(native, two_stage):
        pipe.host_native, pipe.rec_two_stage = native, two_stage
        pipe.stats.clear()
        res = pipe.run_batch(pages, None, det_maps_override=maps)
        assert pipe.stats["t_boxes_ms"] >= 0.0 and pipe.stats["t_db_post_ms"] >= 0.0
        return [r.lines for r in res]

    for two_stage in (True, False):          # per-line widths inside GPU-sized launches / the whole network batch by batch
        a, b = run(True, two_stage), run(False, two_stage)
        assert [len(p) for p in a] == [len(p) for p in b] == [45, 45]
        for pa, pb in zip(a, b):
            for (qa, ta, sa), (qb, tb, sb) in zip(pa, pb):
                qa, qb = np.asarray(qa), np.asarray(qb)
                assert qa.dtype == qb.dtype and qa.tobytes() == qb.tobytes()
                assert ta == tb and type(sa) is type(sb) is float and sa == sb
        assert any(t for p in a for _q, t, _s in p)
