"""Pseudo-labels for box-annotated images: the trained model labels them pixel by pixel under the
constraint of their boxes, and the result is written as TFRecords the per-pixel stream reads.

``python pseudo_label.py <log_dir> <training_problem_def_path> <images_dir> <boxes_json>
<out_tfrecord> {cityscapes,vistas} [--ckpt_path P] [--Nb N] [--results_dir D --export_lids_images
--export_color_decisions]`` plus the model flags, ``--tta_scales`` / ``--tta_flip``,
``--window_canvas`` / ``--window_stride``, ``--crf_*`` and ``--pseudo_tau`` /
``--pseudo_min_fill`` (estimator/pseudo.py; both off by default, neither tuned here).

``boxes_json`` is the index of input_pipelines/train_inputs.py: ``{"<imageid>": [["/m/0k4j",
[xmin, xmax, ymin, ymax]], ...], ...}`` with normalised coordinates, classes through ``MID2CID``
(other mids are dropped), images at ``<images_dir>/<imageid>.jpg``. Images are decoded on the host
and prepared on the device at the network size (the canvas under ``--window_canvas``). A batch is
made of consecutive images (sorted ids) of one size: a size change closes it, and a short batch is
padded with its last image.

Every image becomes one example with ``image/encoded`` (PNG of the raw image), ``label/encoded``
(PNG of ``cids2lids[label]`` at the raw size), ``image/path`` and ``label/path``: what
``parse_cityscapes_example`` reads, so train.py's per-pixel stream and ``evaluate.py
--tfrecords_path`` take ``out_tfrecord`` as it is. ``<out_tfrecord>.report.json`` holds per image
the share of labelled pixels and per box its class, area, hit count and rejected flag.
"""
import json
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np  # noqa: E402

from estimator.mode_keys import ModeKeys  # noqa: E402
from models.resnet50_extended_model_hierarchical import add_model_arguments, model as model_fn  # noqa: E402
from system_factory import SemanticSegmentation  # noqa: E402
from utils.utils import SemanticSegmentationArguments  # noqa: E402


def read_index(path, images_dir):
    """[(imageid, image path, cids int32 [k], coords float32 [k, 4])] in sorted id order."""
    from input_pipelines.train_inputs import MID2CID
    with open(path) as f:
        index = json.load(f)
    out = []
    for iid in sorted(index):
        kept = [(MID2CID[m], c) for m, c in index[iid] if m in MID2CID]
        out.append((iid, os.path.join(images_dir, iid + '.jpg'),
                    np.asarray([k for k, _ in kept], np.int32),
                    np.asarray([c for _, c in kept], np.float32).reshape(len(kept), 4)))
    return out


def pseudo_input(config, params):
    """Batches of Nb consecutive images of one size with their box lists: the features of
    predict_dir_input plus 'boxlists' and 'imageids' (the real images only, like
    'rawimagespaths')."""
    import torch
    from PIL import Image
    from estimator.pseudo import batches_by_size
    from estimator.windows import input_size
    from input_pipelines.tfrecords import prepare_images
    from input_pipelines.utils import get_temp_Nb
    nb = get_temp_Nb(config, params.Nb)
    dev = torch.device('cuda', torch.cuda.current_device())
    entries = read_index(params.boxes_json, params.predict_dir)
    def decode(path):
        with Image.open(path) as im:
            return np.array(im.convert('RGB'), dtype=np.uint8)
    sizes = []
    for _, path, _, _ in entries:   # the header only: the sizes decide the batches
        with Image.open(path) as im:
            sizes.append((im.size[1], im.size[0]))
    for real, padded in batches_by_size(sizes, nb):
        raws = {i: decode(entries[i][1]) for i in real}   # the padding repeats a decoded image
        raw = torch.from_numpy(np.stack([raws[i] for i in padded])).to(dev)
        yield {'proimages': prepare_images(raw, *input_size(params)), 'rawimages': raw,
               'rawimagespaths': [entries[i][1] for i in real],
               'imageids': [entries[i][0] for i in real],
               'boxlists': [(entries[i][2], entries[i][3], sizes[i]) for i in padded]}, None


def build_arguments():
    from estimator.crf import add_crf_arguments
    from estimator.pseudo import add_pseudo_arguments
    from estimator.tta import add_tta_arguments
    from estimator.windows import add_window_arguments
    ssargs = SemanticSegmentationArguments(mode=ModeKeys.PREDICT)   # predict_dir is <images_dir>
    a = ssargs.argparser.add_argument
    a('boxes_json', type=str)
    a('out_tfrecord', type=str)
    a('per_pixel_dataset_name', type=str, choices=['vistas', 'cityscapes'])
    a('--export_color_decisions', action='store_true')
    a('--export_lids_images', action='store_true')
    a('--results_dir', type=str, default=None)
    add_model_arguments(ssargs.argparser)
    add_tta_arguments(ssargs.argparser)
    add_window_arguments(ssargs.argparser)
    add_crf_arguments(ssargs.argparser)
    add_pseudo_arguments(ssargs.argparser)
    return ssargs


def main(argv, max_steps=None):
    from PIL import Image
    from estimator.crf import crf_settings
    from estimator.pseudo import label_id_palette, pseudo_example, pseudo_settings
    from estimator.windows import window_settings
    from input_pipelines.tfrecords import write_records
    s = build_arguments().parse_args(argv)
    s.regularization_weight = 0.0
    s.batch_norm_decay = 1.0
    window_settings(s)
    crf_settings(s)
    pseudo_settings(s)   # refuses a bad --pseudo_* value before anything is built
    if s.replace_voids:
        raise ValueError('--replace_voids does not apply to pseudo-labels: the void label is how '
                         'they say "do not train on this pixel"')
    if s.export_lids_images or s.export_color_decisions:
        assert s.results_dir is not None and os.path.isdir(s.results_dir), (
            'results_dir must a valid path if export_{lids, color}_images flags are True.')
    system = SemanticSegmentation({'predict': pseudo_input}, model_fn, s)
    pdef = system.settings.training_problem_def
    idspal = label_id_palette(pdef)
    colpal = np.array(pdef['cids2colors'], dtype=np.uint8)
    report = {}

    def examples():   # one at a time: the file is written as the batches come
        for out in system.predict(max_steps=max_steps):
            decs = out['decisions'].cpu().numpy()
            raws = out['rawimages'].cpu().numpy()
            for d, raw, path, iid, rep in zip(decs, raws, out['rawimagespaths'], out['imageids'],
                                              out['pseudo_report']):
                lids = idspal[d]
                report[iid] = rep
                if s.export_lids_images:
                    f = os.path.join(s.results_dir, iid + '_pseudo_lids.png')
                    assert not os.path.exists(f), f'Output filename ({f}) already exists.'
                    Image.fromarray(lids).save(f)
                if s.export_color_decisions:
                    f = os.path.join(s.results_dir, iid + '_pseudo_color.png')
                    assert not os.path.exists(f), f'Output filename ({f}) already exists.'
                    Image.fromarray(colpal[d]).save(f)
                yield pseudo_example(raw, lids, path, f'{iid}_pseudo_lids.png')

    write_records(s.out_tfrecord, examples())
    with open(s.out_tfrecord + '.report.json', 'w') as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(f'{len(report)} pseudo-labelled examples -> {s.out_tfrecord}')
    return len(report)


if __name__ == '__main__':
    main(sys.argv[1:])
