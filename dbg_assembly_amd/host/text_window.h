// text_window.h -- what the DBGK_TEXT=device routes of the programs share (clean_common.h, correct_error_reads.cpp, kmerfreq.cpp, map_common.h): the
// switch itself, and the decompressed bytes of an input file window by window for dbgk_parse_chunk -- zlib's gzread (plain and
// ordinary gzip alike; DBGK_GUNZIP is not looked at), what the window before left unconsumed in front of the new bytes, the refusal
// of a record that does not end within 2 GiB of text, and the text_window test hook.
#pragma once

#include "cli_common.h"
#include "dbgk_env.h"

static bool text_on_device()
{
	const char *e = getenv("DBGK_TEXT");
	return e && strcmp(e, "device") == 0;
}

struct TextWindows {
	gzFile in = nullptr;
	string path;
	size_t window = (size_t)256 << 20;
	vector<char> chunk;
	size_t have = 0;    // bytes the window before left unconsumed, at the front of `chunk`
	size_t n_text = 0;  // bytes of the current text
	bool last = false;  // the current text ends the file
	uint64_t windows = 0;

	// window_bytes: the program's own window, where it has a reason for another one than 256 MiB
	explicit TextWindows(const string &in_path, size_t window_bytes = 0) : path(in_path)
	{
		if (window_bytes) window = window_bytes;
		if (const char *h = dbgk_hook("text_window")) // (tests: windows that end inside records of small files; every value gives the same files)
			if (atoll(h) > 0) window = (size_t)atoll(h);
		in = gzopen(path.c_str(), "rb");
	}
	TextWindows(const TextWindows &) = delete;
	TextWindows &operator=(const TextWindows &) = delete;
	~TextWindows()
	{
		if (in) gzclose(in);
	}
	bool ok() const { return in != nullptr; }
	const char *text() const { return chunk.data(); }

	// The next text: the unconsumed tail and up to `window` new bytes.  false once the text that ended the file has been handed out.
	bool next()
	{
		if (last) return false;
		if (have + window >= ((size_t)1 << 31)) {
			cerr << "a record of " << path << " does not end within 2 GiB of text: DBGK_TEXT=device cannot read this file" << endl;
			exit(1);
		}
		chunk.resize(have + window);
		size_t got = 0;
		while (got < window) {
			const int r = gzread(in, chunk.data() + have + got, (unsigned)min<size_t>(window - got, 1u << 30));
			if (r < 0) {
				cerr << "fail to read input file " << path << endl;
				exit(1);
			}
			if (r == 0) {
				last = true;
				break;
			}
			got += (size_t)r;
		}
		n_text = have + got;
		windows++;
		return true;
	}

	// the parser used up `consumed` bytes of the text: the rest goes in front of the next window; a window without a whole record
	// only makes the text longer.  hand_back: the caller itself used less than the parser delivered (map_pair, whose other file gave
	// fewer records): the rest of a text that ended the file is then handed out once more, as the text that ends the file.
	void keep_from(uint64_t consumed, bool hand_back = false)
	{
		if (hand_back && last && consumed < n_text) last = false; // (the next gzread returns 0 again)
		have = last ? 0 : n_text - (size_t)consumed;
		if (have && consumed) memmove(chunk.data(), chunk.data() + consumed, have);
	}
};
