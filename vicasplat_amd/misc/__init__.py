"""The reference's src/misc, as far as it is built: utils (depth and confidence colour maps) and image_io (PNG files made on the device)."""
