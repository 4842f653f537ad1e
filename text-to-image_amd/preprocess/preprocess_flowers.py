"""Oxford-102 flowers: the `<size>images.pickle` stores of train/ and test/ from the JPEGs (reference preprocess/preprocess_flowers.py).

    python -m t2i_amd.preprocess.preprocess_flowers --dir ./data/flowers/ [--load-size 600] [--stage-sizes 4 8 16 38 76 152 304]
                                                    [--force] [--chunk-mb 256] [--workers 8]

For each split the file list is `<split>/filenames.pickle` (a joblib dump), image `key` is `<dir>/<key>.jpg`; every image is
bytescaled and resized to load-size x load-size as the reference's get_image does, on the GPU (preprocess/image_store.py), and the
uint8 [N, S, S, 3] array is written with joblib.dump in file-list order.  --stage-sizes hands the finished array to
stage_images.resize_store in the same run and writes those stores too.  Every argument and file check runs before any device
work; existing stores are kept unless --force; without a GPU the command raises (there is no CPU path)."""
import argparse
import os

from . import image_store as IS

LOAD_SIZE = 600
SPLITS = ('train', 'test')


def load_filenames(data_dir):
    import joblib
    filepath = os.path.join(data_dir, 'filenames.pickle')
    if not os.path.isfile(filepath):
        raise FileNotFoundError('preprocess_flowers: %s does not exist' % filepath)
    filenames = list(joblib.load(filepath))
    print('%s: %d image names' % (filepath, len(filenames)))
    return filenames


def image_paths(inpath, filenames):
    return ['%s/%s.jpg' % (inpath, key) for key in filenames]


def save_data_list(inpath, outpath, filenames, load_size=LOAD_SIZE, stage_sizes=(), force=True, chunk_mb=256, workers=8, device=None):
    """The reference's name: writes the stores of the split directory `outpath` (inside `inpath`) -> {path: shape}."""
    split = os.path.basename(os.path.normpath(outpath))
    paths = image_paths(inpath, filenames)
    IS.check_files('preprocess_flowers', paths)
    return IS.write_split('preprocess_flowers', inpath, split, paths, None, load_size, list(stage_sizes), force, chunk_mb << 20,
                          workers, device or IS.LazyDevice())


def convert_flowers_dataset_pickle(inpath, load_size=LOAD_SIZE, stage_sizes=(), force=True, chunk_mb=256, workers=8):
    """Every check of both splits first, then train/ and test/.  (Called as the reference calls it, with the directory alone, it
    rewrites the load-size stores as the reference does.)"""
    stage_sizes = IS.check_sizes('preprocess_flowers', load_size, stage_sizes)
    names = {split: load_filenames(os.path.join(inpath, split)) for split in SPLITS}
    for split in SPLITS:
        IS.check_files('preprocess_flowers', image_paths(inpath, names[split]))
    device, written = IS.LazyDevice(), {}
    for split in SPLITS:
        written.update(save_data_list(inpath, os.path.join(inpath, split), names[split], load_size, stage_sizes, force, chunk_mb,
                                      workers, device))
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m t2i_amd.preprocess.preprocess_flowers', description=__doc__.split('\n\n')[0])
    IS.add_arguments(ap, LOAD_SIZE)
    args = ap.parse_args(argv)
    IS.check_arguments(ap, args)
    return convert_flowers_dataset_pickle(args.dir, args.load_size, args.stage_sizes, args.force, args.chunk_mb, args.workers)


if __name__ == '__main__':
    main()
