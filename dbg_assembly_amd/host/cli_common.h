// cli_common.h -- what every command-line program here uses: die() on a failed C call, the reference's split() and lib-file
// reader, gzip line input and output, and strings laid back to back for the device.
#pragma once
#include <zlib.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "dbgk.h"

using namespace std;

static void die(const char *what, int rc)
{
	cerr << what << " failed: " << dbgk_strerror(rc);
	if (rc == DBGK_ERR_HIP) cerr << " [" << dbgk_last_error() << "]";
	cerr << endl;
	exit(1);
}

// split (map_func.cpp:33-53, the same in link_func.cpp)
[[maybe_unused]] static void split(const string &line, vector<string> &tokens, const char *delim)
{
	size_t i = 0;
	for (;;) {
		i = line.find_first_not_of(delim, i);
		if (i == string::npos) break;
		const size_t j = line.find_first_of(delim, i);
		tokens.push_back(line.substr(i, j == string::npos ? string::npos : j - i));
		if (j == string::npos) break;
		i = j;
	}
}

// reading_lib_file (map_func.cpp:57-77) and reading_para_file (link_func.cpp:75-95): '#' lines and empty lines skipped, the first
// token taken
[[maybe_unused]] static void reading_lib_file(const string &lib_file, vector<string> &files)
{
	ifstream infile(lib_file.c_str());
	if (!infile) cerr << "fail to open input file" << lib_file << endl;
	string line;
	while (getline(infile, line, '\n')) {
		if (!line.empty() && line[0] == '#') continue;
		vector<string> vec_line;
		split(line, vec_line, " \t\n");
		if (vec_line.empty()) continue;
		files.push_back(vec_line[0]);
	}
}

// getline over a plain or gzip file (what igzstream + getline read); a caller with a message of its own for a failed open
// passes report = false and asks ok().  With DBGK_GUNZIP=device in the environment a file that begins with the 16 fixed header bytes
// of a BGZF member (dbgk.h, GZ and INFLATE sections) is inflated on the GPU: it is read raw in windows of kWindow bytes, a window and
// what the one before it left unconsumed is one dbgk_inf_inflate call that delivers at most kText bytes, and getline is served from
// the inflated bytes.  Any other file -- plain text, an ordinary gzip file -- and any other value of the variable go through zlib as
// ever.  Without a usable GPU the device form fails with the library's error: there is no fall-back to zlib.  A member that the
// device refuses ends the program with status 1.  The device form exists where the program is built with DBGK_READER_DEVICE, as
// host/Makefile builds every bin/ program; a test driver of the host readers that does not link libdbgk.so gets the zlib reader alone.
struct LineReader {
	static constexpr size_t kWindow = (size_t)16 << 20, kText = (size_t)64 << 20; // host buffers near the writer's 64 MiB
	gzFile f = nullptr;
	FILE *raw = nullptr; // DBGK_GUNZIP=device
	dbgk_inf_t z = nullptr;
	string name;
	vector<char> buf = vector<char>(1 << 20), in;
	size_t pos = 0, len = 0, in_len = 0;
	uint64_t members_done = 0;
	bool eof = false, raw_eof = false;
	explicit LineReader(const string &path, bool report = true) : name(path)
	{
#ifdef DBGK_READER_DEVICE
		const char *form = getenv("DBGK_GUNZIP");
		if (form && strcmp(form, "device") == 0 && open_device()) return;
#endif
		f = gzopen(path.c_str(), "rb");
		if (f) gzbuffer(f, 1 << 20);
		else if (report) cerr << "fail to open input file " << path << endl;
	}
	LineReader(const LineReader &) = delete;
	LineReader &operator=(const LineReader &) = delete;
	~LineReader()
	{
		if (f) gzclose(f);
#ifdef DBGK_READER_DEVICE
		if (z) dbgk_inf_destroy(z);
#endif
		if (raw) fclose(raw);
	}
	bool ok() const { return f != nullptr || raw != nullptr; }
#ifdef DBGK_READER_DEVICE
	// the file is this framing by its first 18 bytes: it stays open raw and a handle exists
	bool open_device()
	{
		static const unsigned char head[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
		raw = fopen(name.c_str(), "rb");
		if (!raw) return false;
		in.resize(kWindow + (1 << 16));
		in_len = fread(in.data(), 1, 18, raw);
		if (in_len != 18 || memcmp(in.data(), head, 16) != 0) {
			fclose(raw);
			raw = nullptr;
			in.clear();
			in.shrink_to_fit();
			in_len = 0;
			return false;
		}
		const int rc = dbgk_inf_create(kText, &z);
		if (rc) die("dbgk_inf_create", rc);
		return true;
	}
	// the next window's text into buf; false at the end of the file
	bool refill_device()
	{
		for (;;) {
			if (!raw_eof && in_len < kWindow) {
				const size_t room = kWindow - in_len, n = fread(in.data() + in_len, 1, room, raw);
				in_len += n;
				if (n < room) raw_eof = true;
			}
			if (in_len == 0) return false;
			dbgk_inf_info info;
			int rc = dbgk_inf_inflate(z, in.data(), in_len, raw_eof ? 1 : 0, &info);
			if (rc) {
				cerr << "fail to inflate input file " << name << ": " << dbgk_last_error() << endl;
				die("dbgk_inf_inflate", rc);
			}
			if (info.n_bad) {
				const string what = "inflate of input file " + name + ": member " + to_string(members_done + info.first_bad) + " refused, reason " +
				                    to_string(info.first_bad_reason) + " (DBGK_INF_* of dbgk.h): dbgk_inf_inflate";
				die(what.c_str(), DBGK_ERR_ARG);
			}
			if (info.n_members == 0) die("dbgk_inf_inflate (a window without a whole member)", DBGK_ERR_STATE);
			buf.resize(max<size_t>(info.out_bytes, 1));
			rc = dbgk_inf_results(z, buf.data(), buf.size());
			if (rc) die("dbgk_inf_results", rc);
			members_done += info.n_members;
			memmove(in.data(), in.data() + info.consumed, in_len - info.consumed);
			in_len -= info.consumed;
			pos = 0;
			len = info.out_bytes;
			if (len) return true; // (else: end markers only)
		}
	}
#else
	bool refill_device() { return false; }
#endif
	bool getline(string &s)
	{
		s.clear();
		bool any = false;
		for (;;) {
			if (pos == len) {
				if (eof || !ok()) return any;
				if (raw) {
					if (!refill_device()) { eof = true; return any; }
				} else {
					const int n = gzread(f, buf.data(), (unsigned)buf.size());
					if (n <= 0) { eof = true; return any; }
					pos = 0;
					len = (size_t)n;
				}
			}
			any = true;
			const char *b = buf.data() + pos;
			const char *nl = (const char *)memchr(b, '\n', len - pos);
			if (nl) {
				s.append(b, nl - b);
				pos += (nl - b) + 1;
				return true;
			}
			s.append(b, len - pos);
			pos = len;
		}
	}
};

// what ogzstream writes.  With DBGK_GZ=device in the environment the same text leaves as BGZF-framed gzip members deflated on the
// GPU (dbgk.h, GZ section): it gathers in a host buffer of kWindow bytes, a full buffer is one dbgk_gz_deflate call whose members
// are written as they come back, and close() writes the rest and the end marker.  zlib's readers inflate both forms to the same
// bytes.  Without a usable GPU that form fails with the library's error: there is no fall-back to zlib.  A file that cannot be
// opened is reported and nothing is deflated for it, as the zlib form drops its writes.  A failed device call or a short write ends
// the program with status 1 from write() or close(); the programs call close() themselves, and the destructor of a writer that is
// still open only closes the file and says that its output is incomplete -- it deflates nothing and does not exit.
struct GzWriter {
	static constexpr size_t kWindow = (size_t)1028 * DBGK_GZ_PIECE; // whole pieces, 64 MiB
	gzFile f = nullptr;
	FILE *raw = nullptr; // DBGK_GZ=device
	dbgk_gz_t z = nullptr;
	string name, pending;
	vector<char> members;
	explicit GzWriter(const string &path) : name(path)
	{
		const char *form = getenv("DBGK_GZ");
		if (form && strcmp(form, "device") == 0) {
			raw = fopen(path.c_str(), "wb");
			if (!raw) {
				cerr << "fail to open output file " << path << endl;
				return;
			}
			const int rc = dbgk_gz_create(DBGK_GZ_MAX_LEVEL, &z);
			if (rc) die("dbgk_gz_create", rc);
			return;
		}
		f = gzopen(path.c_str(), "wb");
		if (!f) cerr << "fail to open output file " << path << endl;
	}
	GzWriter(const GzWriter &) = delete;
	GzWriter &operator=(const GzWriter &) = delete;
	~GzWriter()
	{
		if (f) gzclose(f);
		if (z) {
			cerr << "output file " << name << " was not closed: it is incomplete" << endl;
			dbgk_gz_destroy(z);
		}
		if (raw) fclose(raw);
	}
	void write_failed()
	{
		cerr << "fail to write output file " << name << endl;
		exit(1);
	}
	void deflate_pending(bool last)
	{
		dbgk_gz_info info;
		int rc = dbgk_gz_deflate(z, pending.data(), pending.size(), last ? 1 : 0, &info);
		if (rc) die("dbgk_gz_deflate", rc);
		members.resize(info.out_bytes);
		rc = dbgk_gz_results(z, members.data(), members.size());
		if (rc) die("dbgk_gz_results", rc);
		if (!members.empty() && fwrite(members.data(), 1, members.size(), raw) != members.size()) write_failed();
		pending.clear();
	}
	void close()
	{
		if (f) gzclose(f);
		f = nullptr;
		if (z) {
			deflate_pending(true);
			dbgk_gz_destroy(z);
			z = nullptr;
		}
		FILE *file = raw;
		raw = nullptr;
		if (file && fclose(file) != 0) write_failed();
	}
	void write(const char *p, size_t n)
	{
		if (z) {
			while (n) {
				const size_t take = min(n, kWindow - pending.size());
				pending.append(p, take);
				p += take;
				n -= take;
				if (pending.size() == kWindow) deflate_pending(false);
			}
			return;
		}
		for (size_t at = 0; f && at < n; at += 1u << 30) gzwrite(f, p + at, (unsigned)min<size_t>(n - at, 1u << 30));
	}
	void write(const string &s) { write(s.data(), s.size()); }
	// n bytes of text in device memory, behind everything written so far: 16-byte aligned, in whole 16-byte vectors with 64 readable
	// bytes behind them, as the FORMAT and ROWS stages of dbgk.h leave theirs.  With DBGK_GZ=device what the writer still holds on the
	// host is deflated first (a short member in mid-file is valid), then the text where it lies, in slices of whole pieces below 2^31
	// bytes; the end marker stays close()'s.  Otherwise host_copy(dst, n) brings the same bytes to the host for zlib.
	template <class HostCopy>
	void write_device(const void *d_text, uint64_t n, HostCopy host_copy)
	{
		if (!n) return;
		if (!z) {
			vector<char> host(n);
			host_copy(host.data(), host.size());
			write(host.data(), host.size());
			return;
		}
		if (!pending.empty()) deflate_pending(false);
		const uint64_t slice = (uint64_t)32768 * DBGK_GZ_PIECE; // 16-byte aligned offsets: a piece is 16 * 4080 bytes
		static_assert((uint64_t)32768 * DBGK_GZ_PIECE < (1ull << 31) && DBGK_GZ_PIECE % 16 == 0, "a slice is one call on aligned text");
		for (uint64_t at = 0; at < n; at += slice) {
			dbgk_gz_info info;
			int rc = dbgk_gz_deflate_device(z, (const char *)d_text + at, min<uint64_t>(slice, n - at), 0, &info);
			if (rc) die("dbgk_gz_deflate_device", rc);
			members.resize(info.out_bytes);
			rc = dbgk_gz_results(z, members.data(), members.size());
			if (rc) die("dbgk_gz_results", rc);
			if (!members.empty() && fwrite(members.data(), 1, members.size(), raw) != members.size()) write_failed();
		}
	}
	// the text of a formatter's last call (FORMAT section of dbgk.h)
	void write_device(dbgk_fmt *text)
	{
		const void *d_text = nullptr;
		uint64_t n = 0;
		int rc = dbgk_fmt_device(text, &d_text, &n);
		if (rc) die("dbgk_fmt_device", rc);
		write_device(d_text, n, [&](char *dst, size_t cap) {
			rc = dbgk_fmt_results(text, dst, cap);
			if (rc) die("dbgk_fmt_results", rc);
		});
	}
	// stream 0 .. 2 of a row writer's last call (ROWS section of dbgk.h)
	void write_device(dbgk_maprow *rows, int stream)
	{
		const void *d_text = nullptr;
		uint64_t n = 0;
		int rc = dbgk_maprow_device(rows, stream, &d_text, &n);
		if (rc) die("dbgk_maprow_device", rc);
		write_device(d_text, n, [&](char *dst, size_t cap) {
			rc = dbgk_maprow_results(rows, stream, dst, cap);
			if (rc) die("dbgk_maprow_results", rc);
		});
	}
};

// the strings of v back to back, string i at bases[offsets[i] .. offsets[i + 1])
[[maybe_unused]] static void concat(const vector<string> &v, string &bases, vector<uint64_t> &offsets)
{
	bases.clear();
	offsets.assign(1, 0);
	for (const string &s : v) {
		bases += s;
		offsets.push_back(bases.size());
	}
}
