"""Frames without an annotation stop being keyframes (reference data/update_is_det_keyframe.py): after the
opening removed emptied annotations, an image none refers to gets `is_det_keyframe = False`, so
COCOImageDataset, which lists keyframes only, no longer offers it.  Host only."""
from __future__ import annotations

import argparse
import json
import logging
import sys
from pathlib import Path
from typing import Dict, Set

logger = logging.getLogger(__name__)


def get_images_with_annotations(annotations: list) -> Set[int]:
    return {ann["image_id"] for ann in annotations}


def update_is_det_keyframe(coco_data: Dict, dry_run: bool = False) -> Dict:
    """in place; a dry run only reports.  Images already marked False are left alone and not counted."""
    annotated = get_images_with_annotations(coco_data["annotations"])
    updated = 0
    for image in coco_data["images"]:
        if image["id"] in annotated or not image.get("is_det_keyframe", True):
            continue
        if dry_run:
            logger.info("Would update image_id %s: %s -> is_det_keyframe=false", image["id"],
                        image.get("file_name", "unknown"))
        else:
            image["is_det_keyframe"] = False
        updated += 1
    logger.info("Updated %d images to is_det_keyframe=false", updated)
    return coco_data


def process_coco_file(file_path, backup: bool = True, dry_run: bool = False) -> None:
    """rewrite `file_path` (indent 2), after copying it to `<name>.json.backup` when asked"""
    file_path = Path(file_path)
    if backup:
        backup_path = file_path.with_suffix(".json.backup")
        backup_path.write_text(file_path.read_text())
        logger.info("Created backup: %s", backup_path)
    with open(file_path) as f:
        coco_data = json.load(f)
    update_is_det_keyframe(coco_data, dry_run)
    if not dry_run:
        with open(file_path, "w") as f:
            json.dump(coco_data, f, indent=2)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Set is_det_keyframe to false for images without annotations")
    parser.add_argument("files", nargs="+", help="COCO JSON files to update in place")
    parser.add_argument("--no-backup", action="store_true", help="do not write <name>.json.backup first")
    parser.add_argument("--dry-run", action="store_true", help="report what would change, write nothing")
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    missing = [f for f in args.files if not Path(f).exists()]
    if missing:
        logger.error("File not found: %s", ", ".join(missing))
        sys.exit(1)
    for f in args.files:
        process_coco_file(f, backup=not args.no_backup, dry_run=args.dry_run)


if __name__ == "__main__":
    main()
