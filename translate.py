#!/usr/bin/env python3
"""`python translate.py --checkpoint RUN_OR_PTH --input FILE_OR_DIR --output DIR ...` — apply a trained generator to whole
images of any size.  The implementation lives in vae-cyclegan-implementation_amd/translate.py."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
_impl = importlib.import_module("vae-cyclegan-implementation_amd.translate")
load_generator, translate_images, sample_images, build_parser, main = (_impl.load_generator, _impl.translate_images, _impl.sample_images,
                                                                        _impl.build_parser, _impl.main)
interpolate_images = _impl.interpolate_images

if __name__ == "__main__":
    sys.exit(main())
