"""CUB-200-2011 birds: the `<size>images.pickle` stores of train/ and test/ from the JPEGs (reference preprocess/preprocess_birds.py).

    python -m t2i_amd.preprocess.preprocess_birds --dir ./data/birds/ [--load-size 360] [--stage-sizes 4 8 16 38 76 152 304]
                                                  [--force] [--chunk-mb 256] [--workers 8]

For each split the file list is `<split>/filenames.pickle` (a plain pickle), image `key` is `<dir>/CUB_200_2011/images/<key>.jpg`
and its box is the line of `CUB_200_2011/bounding_boxes.txt` that matches its line of `CUB_200_2011/images.txt`.  Every image is
cropped to a square around its box (custom_crop), bytescaled and resized to load-size x load-size as the reference's get_image
does, on the GPU (preprocess/image_store.py); the uint8 [N, S, S, 3] array is written with joblib.dump in file-list order.
--stage-sizes hands the finished array to stage_images.resize_store in the same run.  Every argument and file check (both file
lists, every image file, a box for every key) runs before any device work; existing stores are kept unless --force; without a
GPU the command raises (there is no CPU path)."""
import argparse
import os
import pickle

from . import image_store as IS

LOAD_SIZE = 360
SPLITS = ('train', 'test')


def load_filenames(data_dir):
    filepath = os.path.join(data_dir, 'filenames.pickle')
    if not os.path.isfile(filepath):
        raise FileNotFoundError('preprocess_birds: %s does not exist' % filepath)
    with open(filepath, 'rb') as f:
        filenames = list(pickle.load(f))
    print('%s: %d image names' % (filepath, len(filenames)))
    return filenames


def _rows(path, columns):
    if not os.path.isfile(path):
        raise FileNotFoundError('preprocess_birds: %s does not exist' % path)
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != columns:
                raise ValueError('preprocess_birds: %s line %d has %d fields, expected %d' % (path, ln, len(parts), columns))
            rows.append(parts)
    return rows


def load_bbox(data_dir):
    """-> {image name without '.jpg': [x-left, y-top, width, height] as ints}; the two files are joined line by line."""
    boxes = _rows(os.path.join(data_dir, 'CUB_200_2011/bounding_boxes.txt'), 5)
    names = _rows(os.path.join(data_dir, 'CUB_200_2011/images.txt'), 2)
    if len(boxes) != len(names):
        raise ValueError('preprocess_birds: bounding_boxes.txt has %d lines and images.txt %d' % (len(boxes), len(names)))
    filenames = [n[1] for n in names]
    print('%d bounding boxes read' % len(filenames))
    return {name[:-4]: [int(float(v)) for v in box[1:]] for name, box in zip(filenames, boxes)}


def image_paths(inpath, filenames):
    return ['%s/CUB_200_2011/images/%s.jpg' % (inpath, key) for key in filenames]


def _boxes(filenames, filename_bbox):
    missing = [key for key in filenames if key not in filename_bbox]
    if missing:
        raise KeyError('preprocess_birds: %d of %d images have no bounding box, the first: %s' % (len(missing), len(filenames), missing[0]))
    return [filename_bbox[key] for key in filenames]


def save_data_list(inpath, outpath, filenames, filename_bbox, load_size=LOAD_SIZE, stage_sizes=(), force=True, chunk_mb=256, workers=8,
                   device=None):
    """The reference's name: writes the stores of the split directory `outpath` (inside `inpath`) -> {path: shape}."""
    split = os.path.basename(os.path.normpath(outpath))
    paths, boxes = image_paths(inpath, filenames), _boxes(filenames, filename_bbox)
    IS.check_files('preprocess_birds', paths)
    return IS.write_split('preprocess_birds', inpath, split, paths, boxes, load_size, list(stage_sizes), force, chunk_mb << 20, workers,
                          device or IS.LazyDevice())


def convert_birds_dataset_pickle(inpath, load_size=LOAD_SIZE, stage_sizes=(), force=True, chunk_mb=256, workers=8):
    """Every check of both splits first, then train/ and test/.  (Called as the reference calls it, with the directory alone, it
    rewrites the load-size stores as the reference does.)"""
    stage_sizes = IS.check_sizes('preprocess_birds', load_size, stage_sizes)
    filename_bbox = load_bbox(inpath)
    names = {split: load_filenames(os.path.join(inpath, split)) for split in SPLITS}
    for split in SPLITS:
        _boxes(names[split], filename_bbox)
        IS.check_files('preprocess_birds', image_paths(inpath, names[split]))
    device, written = IS.LazyDevice(), {}
    for split in SPLITS:
        written.update(save_data_list(inpath, os.path.join(inpath, split), names[split], filename_bbox, load_size, stage_sizes, force,
                                      chunk_mb, workers, device))
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m t2i_amd.preprocess.preprocess_birds', description=__doc__.split('\n\n')[0])
    IS.add_arguments(ap, LOAD_SIZE)
    args = ap.parse_args(argv)
    IS.check_arguments(ap, args)
    return convert_birds_dataset_pickle(args.dir, args.load_size, args.stage_sizes, args.force, args.chunk_mb, args.workers)


if __name__ == '__main__':
    main()
